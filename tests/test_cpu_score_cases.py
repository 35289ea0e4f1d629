"""The score checker, reference and host surface of the generation scores, without a GPU.

  * score_cases.check_scores reports every defect of score_cases.DEFECTS at the cap (C_ENT =
    C_LSE = 64), and accepts the reference itself and the stated operation order in numpy fp32;
  * the stated fp32 formula stays within C_ENT of the float64 reference over four method A cases
    whose entropies span 0 to ~5 nats (so the bound leaves a device measurement room);
  * keyword domains: bits_per_sample, Generator.score, gen_persistent_rows, the session level /
    flag pairing, a session without scores=True refusing scores;
  * the new entry points are exported and the new ops registered with fake kernels.
"""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import gen_cases as G
import score_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# three ragged-batch cases of the (16, 2) model and one forced along a stream not its own
CASES = [G.case((16, 2), 64, 'fp32', 9, n) for n in (1, 2, 3)] + \
        [G.case((16, 2), 64, 'fp32', 9, 2, forced='mixed')]
# a ragged last group of four rows (rows 8..11), for the row-swap defect
CASE12 = G.case((16, 2), 64, 'fp32', 12, 2)


def _ref(c):
    model, cond, spk, noise, prefix, n_forced, ref = G.inputs(c)
    return ref, noise, n_forced


# ---------------------------------------------------------------------------- reference, bound
def test_reference_is_the_dense_logp_gathered_and_its_entropy():
    ref, _, _ = _ref(CASES[1])
    sc = S.reference_scores(ref)
    L = S.lookback(ref)
    B, T, Q = ref.logp.shape
    assert sc.shape == (B, T, 2) and sc.dtype == np.float64
    for b, t in ((0, 0), (3, 17), (8, T - 1)):
        assert sc[b, t, 0] == ref.logp[b, t, ref.seq[b, L + t]]
        p = np.exp(ref.logp[b, t])
        assert abs(sc[b, t, 1] - -(p * ref.logp[b, t]).sum()) < 1e-12
    assert (sc[..., 0] <= 0).all() and (sc[..., 1] >= 0).all()
    assert sc[..., 1].max() <= math.log(256) + 1e-12


def test_forced_steps_score_the_forced_sample():
    ref, noise, n_forced = _ref(CASES[3])
    L = S.lookback(ref)
    B, T, _ = ref.logp.shape
    forced = ~G.forced_margin_mask(B, T, n_forced)
    draw = np.argmax(ref.logits - np.log(np.transpose(noise, (1, 0, 2)).astype(np.float64)), -1)
    assert forced.any() and (ref.seq[:, L:][forced] != draw[forced]).all()
    sc = S.reference_scores(ref)
    want = np.take_along_axis(ref.logp, ref.seq[:, L:, None], -1)[..., 0]
    assert np.array_equal(sc[..., 0], want)


def test_stated_fp32_formula_is_within_the_bound():
    """The operations sampler.hpp states, in numpy fp32 (index-order sums), against the float64
    reference: the entropy's largest deviation in the checker's unit leaves C_ENT room, and the
    cases span the entropy range."""
    worst, lo, hi = 0.0, np.inf, 0.0
    for c in CASES:
        ref, _, _ = _ref(c)
        L = S.lookback(ref)
        got = S.fp32_scores(ref.logits, ref.seq[:, L:])
        assert S.check_scores(got, ref) == [], c.id
        want = S.reference_scores(ref)
        worst = max(worst, S.units(got, want)[..., 1].max())
        lo, hi = min(lo, want[..., 1].min()), max(hi, want[..., 1].max())
        # the log-prob is the dense row's element: the same fp32 operations
        z = ref.logits.astype(np.float32)
        m = z.max(-1, keepdims=True)
        dense = (z - m) - np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=np.float32))
        assert np.array_equal(got[..., 0],
                              np.take_along_axis(dense, ref.seq[:, L:, None], -1)[..., 0])
    print('fp32 formula: entropy worst %.2f units, entropies %.3g .. %.3g nats' % (worst, lo, hi))
    assert worst <= S.C_ENT
    assert lo < 0.05 and hi > 4.0


def test_bound_is_capped():
    ref, _, _ = _ref(CASES[0])
    assert S.C_ENT <= S.CAP == 64
    with pytest.raises(AssertionError, match='refused'):
        S.check_scores(S.reference_scores(ref), ref, c_ent=65)
    with pytest.raises(AssertionError, match='refused'):
        S.check_scores(S.reference_scores(ref), ref, c_lse=65)


# ---------------------------------------------------------------------------- defects
@pytest.mark.parametrize('defect', S.DEFECTS)
def test_checker_reports_each_defect_at_the_cap(defect):
    c = CASE12 if defect == 'ragged_swapped' else CASES[3] if defect == 'forced_draw_logp' \
        else CASES[1]
    ref, noise, n_forced = _ref(c)
    assert S.check_scores(S.reference_scores(ref).astype(np.float32), ref, S.CAP, S.CAP) == []
    bad = S.defective(ref, noise, n_forced, defect)
    msgs = S.check_scores(bad, ref, S.CAP, S.CAP)
    assert msgs, defect
    which = ' '.join(msgs)
    if defect in ('entropy_topk', 'entropy_tempered'):
        assert 'entropy' in which and 'log-prob' not in which
    elif defect == 'forced_draw_logp':
        assert 'log-prob' in which and 'entropy' not in which
    else:
        assert 'log-prob' in which and 'entropy' in which


def test_checker_reports_shape_and_negative_entropy():
    ref, _, _ = _ref(CASES[0])
    sc = S.reference_scores(ref).astype(np.float32)
    assert 'shape' in S.check_scores(sc[:, :-1], ref)[0]
    sc[2, 5, 1] = -1e-9
    assert any('negative entropy' in m for m in S.check_scores(sc, ref, S.CAP, S.CAP))


# ---------------------------------------------------------------------------- bits per sample
def test_bits_per_sample_hand_case():
    import model as M
    ln2 = math.log(2.0)
    sc = torch.zeros(2, 4, 2)
    sc[0, :, 0] = torch.tensor([-ln2, -2 * ln2, -3 * ln2, -2 * ln2])          # 1, 2, 3, 2 bits
    sc[1, :, 0] = torch.tensor([-8 * ln2, 0.0, 0.0, -100.0])
    sc[..., 1] = 7.0                                                           # (entropy: unused)
    got = M.bits_per_sample(sc)
    assert got.dtype == torch.float64 and got.shape == (2,)
    assert abs(float(got[0]) - 2.0) < 1e-6 and abs(float(got[1]) - (8 + 100 / ln2) / 4) < 1e-5
    got = M.bits_per_sample(sc, lengths=[2, 3])
    assert abs(float(got[0]) - 1.5) < 1e-6 and abs(float(got[1]) - 8 / 3) < 1e-6
    assert abs(float(M.bits_per_sample(sc.numpy()[0])[0]) - 2.0) < 1e-6        # (T, 2): one row
    assert abs(float(M.bits_per_sample(sc, lengths=1)[1]) - 8.0) < 1e-6
    for bad in ([0, 1], [1, 5], [1, 2, 3]):
        with pytest.raises(ValueError, match='lengths'):
            M.bits_per_sample(sc, lengths=bad)
    with pytest.raises(ValueError, match='scores must be'):
        M.bits_per_sample(torch.zeros(2, 4, 3))


# ---------------------------------------------------------------------------- keyword domains
def test_score_keywords_default_to_the_unscored_call():
    import model as M
    import samplernn_hip as H
    assert inspect.signature(M.Generator.__call__).parameters['return_scores'].default is False
    assert inspect.signature(M.Generator.serve).parameters['scores'].default is False
    assert inspect.signature(M.Generator.session).parameters['scores'].default is False
    assert inspect.signature(M.GenSession.__init__).parameters['scores'].default is False
    assert inspect.signature(H.sample_rows).parameters['return_scores'].default is False
    sig = inspect.signature(M.Generator.score)
    assert list(sig.parameters)[1:] == ['samples', 'cond', 'spk', 'dtype', 'chunk_frames']
    assert sig.parameters['chunk_frames'].default == 0
    # chunk_scored takes what chunk takes
    assert list(inspect.signature(M.GenSession.chunk_scored).parameters) == \
        list(inspect.signature(M.GenSession.chunk).parameters)


def test_score_refuses_bad_arguments_before_any_device_work():
    import model as M
    m = M.SampleRNN([16, 2], 1, 32, True, 256, True, False, 3, 4)
    gen = M.Generator(m)
    cond = torch.zeros(2, 3)                                   # 2 frames, L = 32: 64 samples
    with pytest.raises(ValueError, match='num_cond \\* lookback'):
        gen.score(torch.zeros(1, 63, dtype=torch.long), cond, 0)
    with pytest.raises(ValueError, match='chunk_frames'):
        gen.score(torch.zeros(1, 64, dtype=torch.long), cond, 0, chunk_frames=-1)


def test_session_without_scores_refuses_scores():
    """chunk_scored on a session opened without scores=True raises before anything runs (no
    handle is used, no tensor is made: the object below has neither a model nor a device)."""
    import model as M
    ses = object.__new__(M.GenSession)
    ses._handle, ses.scores = 12345, False
    with pytest.raises(ValueError, match='scores=True'):
        ses.chunk_scored(torch.zeros(1, 1, 3), spk=0)
    ses._handle = None                                          # (so that __del__ closes nothing)


def test_level_and_flag_domains():
    import custom_ops
    import samplernn_hip as H
    assert H.GEN_SESSION_SCORE == 16
    # the scored level is reached through `scores`, not through ctrl
    with pytest.raises(ValueError):
        H.gen_persistent_rows(torch.float32, 8, 64, 16, ctrl=3)
    # level 3 and the flag go together: refused before the library is asked
    for level, flags in ((3, 0), (0, 16), (2, 16 | 1), (4, 16)):
        with pytest.raises(ValueError):
            custom_ops.gen_session_open([], [], 1, 1, level, 0, 0, flags)
    dll = H.lib().dll
    sz = ctypes.c_size_t(0)
    m = H.SrnnModel()
    for level, flags in ((3, 0), (0, 16), (1, 16), (3, 32 | 16), (4, 16)):
        assert dll.srnn_gen_session_bytes(ctypes.byref(m), 1, 1, level, flags,
                                          ctypes.byref(sz)) == 1
        want = b'go together' if level <= 3 and flags < 32 else b'bad args'
        assert want in dll.srnn_last_error(), (level, flags, dll.srnn_last_error())
    # the plan answers for level 3, and not above it
    fn = dll.srnn_gen_persistent_rows_level
    fn.argtypes = [ctypes.c_int] * 6
    assert fn(H.dcode(torch.float32), 8, 64, 16, 256, 4) == 0


# model.generation_weights' layout integers of the (16, 2) model at D = 64, cond_dim 3, fp32:
# n_tiers, n_rnn, dim, q_levels, cond_dim, dtype, then (frame_size, n_frame_samples, in_dim,
# has_input_expand) per tier, then the lookback
META = [2, 1, 64, 256, 3, 0, 16, 16, 16, 1, 2, 32, 35, 0, 32]


def _layout_struct():
    """An SrnnModel with the layout integers only (what the size queries read)."""
    import samplernn_hip as H
    m = H.SrnnModel()
    m.n_tiers, m.n_rnn, m.dim, m.q_levels, m.cond_dim, m.dtype = META[:6]
    for k in range(m.n_tiers):
        t = m.tier[k]
        t.frame_size, t.n_frame_samples, t.in_dim, _ = META[6 + 4 * k: 10 + 4 * k]
        t.b_up = 1
    return m


def test_session_arena_grows_by_eight_bytes_per_row_step():
    """srnn_gen_session_bytes with the flag = the level-2 arena + steps * n_seqs * 8 (rounded up
    to the arena's 256-byte granule); the level-3 control arrays are level 2's."""
    import samplernn_hip as H
    sm = _layout_struct()
    dll = H.lib().dll
    fn = dll.srnn_gen_session_bytes
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_size_t)]
    for B, F in ((9, 3), (1, 1), (17, 2)):
        a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert fn(ctypes.byref(sm), B, F, 2, 1, ctypes.byref(a)) == 0, dll.srnn_last_error()
        assert fn(ctypes.byref(sm), B, F, 3, 1 | 16, ctypes.byref(b)) == 0, dll.srnn_last_error()
        grow = F * 32 * B * 8
        assert b.value - a.value == -(-grow // 256) * 256, (B, F, a.value, b.value)


# ---------------------------------------------------------------------------- the surface
def test_library_exports_the_score_entry_points():
    import custom_ops
    import samplernn_hip as H
    dll = ctypes.CDLL(H.LIB_PATH)
    txt = open(os.path.join(ROOT, 'include', 'samplernn_hip.h')).read()
    for name in ('srnn_generate7', 'srnn_sample_rows2', 'srnn_gen_session_chunk2'):
        assert hasattr(dll, name), name
        assert name in H._SIGS and name in H.exported_symbols()
        assert re.search(r'\b%s\s*\(' % name, txt), name
    assert re.search(r'#define\s+SRNN_GEN_SESSION_SCORE\s+16\b', txt)
    assert dll.srnn_abi_version() == 2
    # the older entries' signatures have one argument fewer: generate7 = generate6 + score
    assert H._SIGS['srnn_generate7'][:-1] == H._SIGS['srnn_generate6']
    assert H._SIGS['srnn_sample_rows2'][:-1] == H._SIGS['srnn_sample_rows']
    assert [f[0] for f in H.SrnnGenChunk._fields_][-1] == 'logp_out'      # (not changed)
    for name in ('generate_scored', 'sample_rows_scored', 'gen_session_chunk_scored'):
        assert name in custom_ops.OPS and hasattr(torch.ops.srnn, name)
    # bad arguments are refused without a device
    assert dll.srnn_sample_rows2(None, 256, 1, None, 0, 0, 0, None, None, None, None, None, None,
                                 None) == 1


def test_scored_ops_have_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import custom_ops  # noqa: F401
    weights, meta = [torch.empty(1)], META
    with FakeTensorMode(allow_non_fake_inputs=True):
        idx, lp, sc = torch.ops.srnn.sample_rows_scored(torch.empty(5, 256), None, 0, 0, 0, None,
                                                        None, None, False)
        assert tuple(idx.shape) == (5,) and idx.dtype == torch.int64
        assert tuple(lp.shape) == (0,) and tuple(sc.shape) == (5, 2) and sc.dtype == torch.float32
        _, lp, _ = torch.ops.srnn.sample_rows_scored(torch.empty(5, 256), None, 0, 0, 0, None,
                                                     None, None, True)
        assert tuple(lp.shape) == (5, 256)
        seq, lp, st, sc = torch.ops.srnn.generate_scored(
            weights, meta, torch.empty(3, 2, 3), torch.empty(3, 64), None, 0, 0, 1, False, None,
            None, None, None, 0, None, None, False, None, None)
        assert tuple(seq.shape) == (3, 32 + 64) and tuple(sc.shape) == (64, 3, 2)
        assert tuple(lp.shape) == (0,) and tuple(st.shape) == (0,)
        seq, lp, sc = torch.ops.srnn.gen_session_chunk_scored(
            1, 32, torch.empty(3, 2, 3), None, None, None, None, None, None, None, None, True)
        assert tuple(seq.shape) == (3, 64) and tuple(lp.shape) == (64, 3, 256)
        assert tuple(sc.shape) == (64, 3, 2)
