"""The GRU conformance cases proved on the CPU (gru_cases.py, test_gpu_gru_conformance.py's
tables): every Method A and exact Method C case is exact in fp32 in two summation orders, the
step-local bounds hold for an fp32 evaluation in both orders, the tables lie on both sides of
every dispatcher condition, and the checker reports each of the listed single defects by
element."""
import dataclasses

import pytest
import torch

import gru_cases as G
import test_gpu_gru_conformance as T
from gru_cases import case

ALL = [c for name in sorted(T.TABLES) for c in T.TABLES[name]] + T.ALLOWANCE
TAKES = [c for c in ALL if c.expect == 'takes']


def _ids(cs):
    return [c.id for c in cs]


def test_ids_are_unique():
    ids = _ids(ALL)
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


@pytest.mark.parametrize('c', TAKES, ids=_ids(TAKES))
def test_every_case_holds_in_float32(c):
    """An fp32 evaluation of the case, its k-slices summed ascending or descending, passes the
    case's checker: bit for bit for methods A, C and Crne (build() has asserted the method's
    preconditions in float64), within the derived bounds for B and Cloc."""
    for order in (0, 1):
        t = G.build(c)
        G.evaluate(t, order)
        report = G.check(t)
        assert report is None, 'order %d: %s' % (order, report)
        if c.method == 'B0':
            assert t.stats['fn_err_u'] <= G.C_FN / 2


FWD_A = [c for c in TAKES if c.method == 'A']


@pytest.mark.parametrize('c', FWD_A, ids=_ids(FWD_A))
def test_saturation_and_shares(c):
    """Every r / z / n argument is 0 or beyond +-1000, and every value of z and of n has a
    share of at least a fifth, so h really changes from step to step."""
    t = G.build(c)
    D = c.D
    gi, _ = G.effective_gi(t)
    W, b = t.w['whh'].read2().double(), t.w['bhh'].read2().double().view(-1)
    gates = t.ref['gates']
    h = torch.cat([t.w['h0'].read2().double().view(c.B, 1, D), t.ref['out'][:, :-1]], 1)
    gh = h @ W.t() + b
    arz = gi[..., :2 * D] + gh[..., :2 * D]
    an = gi[..., 2 * D:] + gh[..., 2 * D:] * gates[..., :D]
    assert bool((arz.abs() > 1000).all())
    assert bool(((an == 0) | (an.abs() > 1000)).all())
    z, n = gates[..., D:2 * D], gates[..., 2 * D:3 * D]
    assert bool(((z == 0) | (z == 1)).all()) and bool(((n == 0) | (n.abs() == 1)).all())
    if c.B * c.Fr * D >= 2000:
        for v in (0.0, 1.0):
            assert float((z == v).double().mean()) >= 0.2
        for v in (-1.0, 0.0, 1.0):
            assert float((n == v).double().mean()) >= 0.2
    if c.variant == 'x':        # (b_ih saturates per unit: the same gates at every step)
        assert not torch.equal(t.ref['out'][:, 0], t.w['h0'].read2().double())
    elif c.Fr > 1:
        assert not torch.equal(t.ref['out'][:, 0], t.ref['out'][:, -1])


RNE = [c for c in TAKES if c.method == 'Crne']


@pytest.mark.parametrize('c', RNE[:4], ids=_ids(RNE[:4]))
def test_rne_cases_test_the_rounding_mode(c):
    """Step 1 of a Crne case carries more than 8 significant bits, a good share of its values
    round up, and a truncating store of the hand-off fails the check."""
    t = G.build(c)
    g = t.ref['dgh'][:, 1]
    if c.dtype == 'bf16':
        up = G.bf16r(g).abs() > G.trunc_bf16(g).double().abs()
        assert float(up.double().mean()) > 0.02 and int(up.sum()) > 100
        G.evaluate(t, 0, 'trunc')
        assert 'dghlp' in G.check(t)
    else:
        assert not torch.equal(G.bf16r(g), g)


# ---- the checker bites: single defects built into the evaluation
M_FWD_A = case('fwd', 'xcd2', 'A', 'bf16', 20, 256, 3, 'tm')
M_FWD_B = case('fwd', 'seq', 'B', 'bf16', 33, 128, 3, 'tm')
M_FWD_B32 = case('fwd', 'steps', 'B', 'f32', 17, 80, 3, 'pad')
M_BWD_C = case('bwd', 'xcd2', 'C', 'bf16', 20, 256, 2, 'tm')
M_BWD_R = case('bwd', 'xcd2', 'Crne', 'bf16', 20, 256, 2, 'tm')
M_BWD_L = case('bwd', 'xcd2', 'Cloc', 'bf16', 20, 256, 3, 'tm')
M_BWD_L32 = case('bwd', 'steps', 'Cloc', 'f32', 17, 80, 3, 'pad', variant='both')

MUTATIONS = (
    [(c, 'swap_rz', ('gates', 'block 0')) for c in (M_FWD_A, M_FWD_B, M_FWD_B32)]
    + [(c, 'stale_h', ('gates', 'step 2')) for c in (M_FWD_A, M_FWD_B, M_FWD_B32)]
    + [(c, 'h0_at_1', ('gates', 'step 1')) for c in (M_FWD_A, M_FWD_B, M_FWD_B32)]
    + [(M_FWD_A, 'drop_k', ('gates', 'block 3'))]
    + [(c, 'drop_k', ('gates', 'step 0')) for c in (M_FWD_B, M_FWD_B32)]
    + [(M_FWD_B, 'trunc', ('outlp',))]
    + [(c, 'row_dup', ('row %d' % (c.B - 1),)) for c in (M_FWD_A, M_FWD_B, M_BWD_C, M_BWD_L)]
    + [(M_FWD_A, 'canary', ('outside the out window',)),
       (M_BWD_C, 'canary', ('outside the dgh window',))]
    + [(c, 'drop_k', ('dgh', 'step 0')) for c in (M_BWD_C, M_BWD_R, M_BWD_L, M_BWD_L32)]
    + [(c, 'ddir0_from_1', ('ddir0',)) for c in (M_BWD_C, M_BWD_R, M_BWD_L, M_BWD_L32)]
    + [(c, 'trunc', ('dghlp',)) for c in (M_BWD_R, M_BWD_L)]
    # an error of 1e-4 |dh| in one dh: passes the 2e-2 * max|ref| of the older tests
    + [(c, 'dh_rel', ('row 0',)) for c in (M_BWD_C, M_BWD_R)]
)


@pytest.mark.parametrize('c,mut,names', MUTATIONS,
                         ids=['%s-%s' % (c.id, m) for c, m, _ in MUTATIONS])
def test_checker_reports_the_defect(c, mut, names):
    t = G.build(c)
    G.evaluate(t)
    assert G.check(t) is None
    t = G.build(c)
    G.evaluate(t, 0, mut)
    report = G.check(t)
    assert report is not None, 'the checker passed a kernel with the defect ' + mut
    for n in names:
        assert n in report, report


def test_the_relative_dh_error_passes_the_older_tolerance():
    """The defect Method C must catch is one today's test_gru_xcd_bwd lets through."""
    t = G.build(M_BWD_C)
    G.evaluate(t, 0, 'dh_rel')
    got, ref = t.w['dgh'].read().double(), t.ref['dgh']
    assert float((got - ref).abs().max()) <= 2e-2 * float(ref.abs().max())
    assert G.check(t) is not None


def test_checker_reports_an_unwritten_element_and_a_written_input():
    t = G.build(M_FWD_A)
    G.evaluate(t)
    x = t.w['gates']
    G._ints(x.buf)[int(x.index[5])] = G._canary(x.dtype)
    assert 'were not written' in G.check(t)
    t = G.build(M_FWD_A)
    G.evaluate(t)
    t.w['gi'].buf[0] = 1.0
    assert 'input buffer gi was written' in G.check(t)
    t = G.build(M_BWD_C)
    assert G.untouched(t)
    t.w['ddir0'].buf[-1] = 0.0
    assert not G.untouched(t)


def test_sequence_window():
    """Time-major, padded and offset windows address x[b][t] = base + b ld + t s, keep their
    guards, and see a write into any gap."""
    for lay in G.LAYOUTS:
        c = dataclasses.replace(M_FWD_A, layout=lay)
        ld, s, off = G.strides(c, 'g', 4 * c.D)
        w = G.SeqWindow(torch.float32, c.B, c.Fr, 4 * c.D, ld, s, 'cpu', off)
        v = torch.arange(c.B * c.Fr * 4 * c.D, dtype=torch.float32).view(c.B, c.Fr, -1)
        w.fill(v)
        assert torch.equal(w.read(), v) and w.outside_ok() and w.written()
        assert float(w.buf[w.base + 3 * ld + 2 * s + 7]) == float(v[3, 2, 7])
        assert w.ptr(2) - w.ptr(0) == 2 * s * 4 and (w.ptr(0) - w.buf.data_ptr()) % 16 == off * 4 % 16
        w.buf[w.base - 1] = 0.0
        assert not w.outside_ok() and w.first_outside() == (w.base - 1, 1)
    # the 8-element rule of the seq sweeps holds in every layout they are given
    for lay in ('dense', 'pad', 'tm', 'wide', 'off'):
        c = case('fwd', 'seq', 'A', 'bf16', 33, 128, 3, lay)
        for op, X in (('o', 128), ('d', 384)):
            ld, s, off = G.strides(c, op, X)
            assert ld % 8 == 0 and s % 8 == 0 and off % 8 == 0
    ld, s, off = G.strides(case('fwd', 'seq', 'A', 'bf16', 33, 128, 2, 'odd'), 'o', 128)
    assert ld % 8 != 0


# ---- the tables lie on both sides of every dispatcher condition
def _routes(name, **kw):
    return [(c, G.xcd_route(c)) for c in T.TABLES[name]
            if c.expect == 'takes' and all(getattr(c, k) == v for k, v in kw.items())]


def test_xcd_tables_cover_the_dispatch():
    fwd, bwd = _routes('xcd_fwd'), _routes('xcd_bwd')
    assert all(r is not None and r['chunks'] == 1 for _, r in fwd + bwd)
    # the batch sizes come from the layout rule: MT = 1, 2 and 4 at D = 768 and at D = 256
    for D in (768, 256):
        for mt in (1, 2, 4):
            assert G.gx_layout(T.rows_for(D, mt), D, G.NCU)[0] == mt
            assert G.gx_layout(T.rows_for(D, mt) - 11, D, G.NCU)[0] == max(mt // 2, 1) or mt == 1
    for rs in (fwd, bwd):
        assert {(c.D, r['mt']) for c, r in rs} >= {(D, mt) for D in (768, 256) for mt in (1, 2, 4)}
        assert {c.D for c, _ in rs} == {256, 512, 768, 1024}
        for m in {c.method for c, _ in rs}:
            assert {c.D for c, _ in rs if c.method == m} == {256, 512, 768, 1024}
    # forward: the three unit counts per wave (D = 768: ui = 2 at runtime D), D = 1024 at
    # compile time and, with SRNN_GX_DC=0, at runtime; fewer than 16 rows per tile and 16
    assert {(r['ui'], r['dc']) for _, r in fwd} == {(0, False), (1, False), (2, False), (2, True)}
    assert {(c.D, r['ui'], r['dc']) for c, r in fwd} >= {(768, 2, False), (1024, 2, False),
                                                         (1024, 2, True)}
    assert {r['rv'] for _, r in fwd} >= {1, 2, 3, 16} and {r['rv'] for _, r in bwd} >= {1, 2, 3, 16}
    # backward: packed and unpacked at every D and MT; full == false is D = 768's alone; the
    # batched form on and off wherever MT > 1; the unpacked MT = 4 form needs its LDS raised
    assert {(c.D, r['mt'], r['pk']) for c, r in bwd} >= {
        (D, mt, pk) for D in (768, 256) for mt in (1, 2, 4) for pk in (True, False)}
    assert {(c.D, r['pk']) for c, r in bwd} >= {(D, pk) for D in (256, 512, 768, 1024)
                                                for pk in (True, False)}
    assert {(c.D, r['full']) for c, r in bwd if not r['pk']} == {
        (256, True), (512, True), (768, False), (1024, True)}
    assert {(r['ui']) for c, r in bwd if not r['pk']} == {0, 1, 2}
    assert {(r['mt'], r['batch']) for c, r in bwd if r['pk'] and r['mt'] > 1} == {
        (2, True), (2, False), (4, True), (4, False)}
    lds = {r['lds_unpacked'] > 64 * 1024 for c, r in bwd if not r['pk']}
    assert lds == {True, False}
    # both switches of the hand-off mode, once per direction
    for rs in (fwd, bwd):
        assert any(c.envget('SRNN_GEN_LOCAL') == 0 for c, _ in rs)
    # every layout reaches a packed and an unpacked launch
    assert {(c.layout, r['pk']) for c, r in bwd} >= {(l, pk) for l in ('dense',) + T.FLAYOUTS
                                                     for pk in (True, False)}


def test_two_gigabyte_offsets_take_the_unpacked_kernel():
    """The packed kernel's operand fetch uses 32-bit byte offsets: a launch whose largest
    offset passes 2 GB takes the unpacked one.  Shown here only (nothing is allocated)."""
    c = case('bwd', 'xcd2', 'C', 'bf16', 20, 1024, 2)
    assert G.xcd_route(c)['pk']
    for op in ('dy', 'g', 'o'):
        st = {k: G.strides(c, k, x)[:2] for k, x in (('dy', 1024), ('g', 4096), ('o', 1024))}
        st[op] = (2 ** 25, st[op][1])                  # 19 rows x 2^25 x 4 bytes > 2 GB
        r = G.xcd_route(c, fake_strides=st)
        assert not r['pk'] and r['omax'] >= 0x7fffffff - 64
        st[op] = (2 ** 24, st[op][1])
        assert G.xcd_route(c, fake_strides=st)['pk']


def test_seq_and_layer_tables_cover_their_conditions():
    for name in ('seq_fwd', 'seq_bwd'):
        cs = [c for c in T.TABLES[name] if c.expect == 'takes']
        assert all(G.seq_supported(c) and G.xcd_route(c) is None for c in cs)
        assert {(c.D, c.B) for c in cs} >= {(D, B) for D in (128, 384) for B in (1, 31, 32, 33, 40)}
        assert {G.cdiv(c.B, 32) for c in cs} == {1, 2}
        assert {c.layout for c in cs} == {'dense', 'pad', 'tm', 'wide', 'off'}
        assert {c.Fr for c in cs} >= {1, 2 if name == 'seq_bwd' else 3}
    for name in ('layer_fwd', 'layer_bwd'):
        cs = T.TABLES[name]
        assert all(G.layer_plan(c) == c.plan for c in cs)
        assert {(c.plan, c.dtype) for c in cs} == {('xcd', 'bf16'), ('seq', 'bf16'),
                                                   ('steps', 'bf16'), ('steps', 'f32')}
        # rows(): two launches of 64 + 16 rows, under padded and under time-major strides
        shared = [(c, G.xcd_route(c)) for c in cs if c.share == 8]
        assert {c.layout for c, _ in shared} == {'pad', 'tm'}
        assert all(r['chunks'] == 2 and r['lr'] == 64 and r['mt'] == 4 for _, r in shared)
        assert {c.layout for c in cs if c.share == 1} >= {'dense', 'pad', 'tm'}


def test_steps_tables_cover_the_kernel_choice():
    """launch_cell / launch_bwd take the ring kernel when D is a multiple of the ring stage and
    the streamed operand and the weight are 16-byte aligned with a 16-byte pitch.  The tables
    hold ring-eligible shapes on both sides of the alignment test, per dtype and direction."""
    for name in ('steps_fwd', 'steps_bwd'):
        cs = [c for c in T.TABLES[name] if c.expect == 'takes']
        assert {(c.dtype, c.D, c.B) for c in cs} >= {
            (d, D, B) for d in ('bf16', 'f32') for D in (48, 80, 256) for B in (1, 15, 16, 17, 33)}
        assert {c.Fr for c in cs} >= {1, 2, 3}
        seen = set()
        for c in cs:
            t = G.build(c)
            route = G.steps_route(t)
            if c.D != 256:
                assert not any(route)                     # 48, 80: no multiple of the stage
            else:
                # (a sequence's first forward step reads the dense h0, its last backward
                #  step no dgh_next: the layout decides the steps after them)
                seen.add((c.dtype, c.variant, c.Fr > 1 and route[-1]))
                seen.add((c.dtype, '', c.Fr > 1 and route[-1]))
        for d in ('bf16', 'f32'):
            assert {(d, '', True), (d, '', False)} <= seen
            if name == 'steps_fwd':
                assert {(d, 'x', True), (d, 'x', False), (d, 'wmis', False)} <= seen
            else:
                assert {(d, 'wt', True), (d, 'w', False), (d, 'wmis', False),
                        (d, 'both', True), (d, 'both', False)} <= seen
