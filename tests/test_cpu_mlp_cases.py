"""The exact-arithmetic cases of the MLP / glue conformance sweep proved on the CPU (no GPU):
every case of every table satisfies its builder's preconditions, a float32 evaluation of it
in a deliberately different order equals the float64 reference bit for bit (so a mismatch on
the GPU is the kernel's, not the method's), the case ids are unique, the checker finds a
single changed output element and a single changed canary where they are, the dTab rounding
cases have inexact entries and ties that a truncating store fails, and every table has a case
on each side of the dispatch conditions it is there for (recomputed here from the shapes)."""
import pytest
import torch

import gemm_cases as G
import mlp_cases as C
import test_gpu_mlp_conformance as T


def _solved(family, c):
    build, evaluate = C.FAMILIES[family]
    t = build(c)
    evaluate(t)
    return t


def _check(family, t):
    return C.check_dtab(t, t.colsum_done) if family == 'dtab' else C.check(t)


@pytest.mark.parametrize('name', list(T.TABLES))
def test_every_case_is_exact_in_float32(name):
    """The builders assert their preconditions; the float32 evaluation from the placed
    operands (cast to the case's dtypes, read back out of their windows, summed in another
    order) written into the output windows satisfies the checker, whose expected bits are the
    float64 reference's."""
    family, cases = T.TABLES[name]
    for c in cases:
        t = _solved(family, c)
        assert _check(family, t) is None, c.id
        for k, x in t.w.items():
            assert x.outside_ok(), (c.id, k)


def test_ids_are_unique():
    ids = [c.id for c in T.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert all(' ' not in i for i in ids)


def test_index_windows_are_guarded():
    """Index streams: ldx > W, xoff in {0, 3}, an out-of-range canary everywhere else."""
    seen = set()
    for name in ('l1_generic', 'l1_lds', 'dtab_packed', 'dtab_generic'):
        family, cases = T.TABLES[name]
        for c in cases[:6]:
            x = C.FAMILIES[family][0](c).w['x']
            assert x.ld > x.xoff + x.cols - 1 and x.ld > x.cols and x.xoff in (0, 3)
            assert x.outside_ok() and int(x.buf[0]) == C.XCANARY >= 1 << 32
            assert x.rows == 0 or int(x.read().max()) < c.Q
            seen.add(x.xoff)
    assert seen == {0, 3}
    tg = C.build_nll(T.NLL[0]).w['target']
    assert tg.ld > tg.cols and tg.outside_ok()


ONE_OF_EACH = [('l1', T.L1_GENERIC[1], 'out'), ('l1', T.L1_BITS[-3], 'bits'),
               ('dtab', T.DTAB_DIRECT[1], 'dtab'), ('dtab', T.DTAB_DIRECT[1], 'colsum'),
               ('out_bwd', T.OUT_BWD[0], 'da2'), ('out_bwd', T.OUT_BWD[0], 'csp'),
               ('nll', T.NLL[-1], 'loss'), ('nll', T.NLL[3], 'dlogp'),
               ('glue', T.GLUE[4], 'out'), ('glue', T.GLUE[-2], 'flat')]


@pytest.mark.parametrize('family,c,name', ONE_OF_EACH, ids=[c.id + '.' + n for _, c, n in ONE_OF_EACH])
def test_checker_reports_a_changed_output_element(family, c, name):
    t = _solved(family, c)
    assert _check(family, t) is None
    x = t.w[name]
    i = x.index.numel() // 2
    e = int(x.index[i])
    G._ints(x.buf)[e] ^= 1                                              # one bit of one element
    r = _check(family, t)
    row, col = (e - x.front) // x.ld, (e - x.front) % x.ld
    if name == 'flat':
        row, col = 0, i
    assert 'inside the %s window: 1 of %d elements differ' % (name, x.index.numel()) in r
    assert '(row %d, col %d)' % (row, col) in r and 'outside' not in r and 'got 0x' in r


@pytest.mark.parametrize('family,c,name', ONE_OF_EACH, ids=[c.id + '.' + n for _, c, n in ONE_OF_EACH])
def test_checker_reports_a_changed_canary(family, c, name):
    t = _solved(family, c)
    x = t.w[name]
    keep = torch.ones(x.buf.numel(), dtype=torch.bool)
    keep[x.index] = False
    e = int(keep.nonzero()[-3])                                         # in the guard after it
    x.buf.view(torch.uint8)[e * x.buf.element_size()] ^= 0x10           # one byte of a canary
    r = _check(family, t)
    assert 'outside the %s window: 1 canary elements overwritten' % name in r
    assert 'first at buffer element %d' % e in r and 'inside' not in r


def test_checker_reports_a_written_input_and_gap():
    t = _solved('l1', T.L1_GENERIC[0])
    t.w['x'].buf[1] = 0                                                 # an index canary
    t.w['upper'].buf[0] = 1.0
    r = C.check(t)
    assert 'input buffer x was written' in r and 'input buffer upper was written' in r
    # the gap between two tensors of a packed bucket is a canary like any other
    t = _solved('glue', T.GLUE[-3])
    x = t.w['flat']
    gap = x.front + t.offs[0] + t.sizes[0]
    assert gap not in set(x.index.tolist())
    x.buf[gap] = 0.0
    assert 'outside the flat window: 1 canary' in C.check(t)


def test_untouched_sees_a_write_by_a_declined_call():
    c = [c for c in T.OUT_BWD if not C.out_bwd_served(c)][0]
    t = C.build_out_bwd(c)
    assert C.untouched(t) is None
    t.w['csp'].buf[t.w['csp'].front] = 0.0
    assert 'csp' in C.untouched(t)
    t = C.build_dtab(T.DTAB_POSWS[0])
    C.eval_dtab(t)
    assert not t.colsum_done and C.check_dtab(t, 0) is None
    assert 'colsum_done' in C.check_dtab(t, 1)
    t.w['colsum'].buf[t.w['colsum'].front + 1] = 0.0                    # skipped, yet written
    assert 'colsum was written' in C.check_dtab(t, 0)


def _rounding_cases():
    return [c for c in T.DTAB_PACKED + T.DTAB_GENERIC if c.positive]


def test_dtab_recipe_tests_the_rounding_mode():
    """The `positive` cases have sums that need rounding to bf16, exact ties among them, so
    truncation or round-half-up on the bf16 store cannot pass: over all entries of the small
    generic case, and over the entries of the sample values that occur in the packed one."""
    cases = _rounding_cases()
    assert {C.dtab_route(c) for c in cases} == {'packed', 'generic4'}
    for c in cases:
        t = C.build_dtab(c)
        tab = t.ref['dtab']
        used = torch.bincount(t.values['x'].reshape(-1), minlength=c.Q) > 0
        assert c.Q > 4 or bool(used.all())
        bits = tab[used].float().view(torch.int32)
        inexact = (bits & 0xffff) != 0
        ties = (bits & 0xffff) == 0x8000
        assert float(inexact.float().mean()) > 0.2, c.id
        assert float(ties.float().mean()) > 0.01, c.id
        # a truncating store fails the checker, and is named
        C.eval_dtab(t)
        assert C.check_dtab(t, t.colsum_done) is None
        full = tab.float().view(torch.int32)
        t.w['dtab'].fill((full & ~0xffff).view(torch.float32).to(torch.bfloat16))
        r = C.check_dtab(t, t.colsum_done)
        assert r is not None and 'inside the dtab window' in r


def test_packed_precondition_is_the_kernels():
    """e = min(floor(log2(2^30 / (amax cmax))), 40), cmax over the window positions only."""
    assert C.packed_exponent(3 / 256, 100) == 29 and C.packed_exponent(2.0 ** -20, 1) == 40
    for c in T.DTAB_PACKED:
        if C.dtab_route(c) != 'packed':
            continue
        t = C.build_dtab(c)
        x = t.w['x'].read()
        assert t.cmax == int(torch.bincount(x.reshape(-1), minlength=256).max())
        assert t.e >= 8 and 3 * t.cmax * 2 ** (t.e - 8) < 2 ** 30
    skew = C.build_dtab(T.DTAB_PACKED[2])
    assert skew.case.dist == 'skew' and skew.cmax > 0.5 * skew.w['x'].index.numel()


def test_l1_tables_cover_the_dispatch():
    r = lambda cs: [C.l1_route(c) for c in cs]                          # noqa: E731
    assert set(r(T.L1_GENERIC)) == {'generic'}
    by = {c.id: C.l1_route(c) for c in T.L1_XCD + T.L1_LDS + T.L1_BITS}
    f = lambda *a, **k: by[C.l1case(*a, **k).id]                        # noqa: E731
    # rows >= 4096 is the threshold; rows need not be a multiple of 64
    assert f('f32', 'f32', 4, 1024, 128) == 'xcd' and f('f32', 'f32', 3, 1365, 128) == 'generic'
    assert f('bf16', 'f32', 5, 820, 256) == 'xcd' and (5 * 820) % 64 != 0
    for d, u in (('f32', 'f32'), ('bf16', 'f32')):
        assert f(d, u, 4, 1024, 128, places={'upper': 'pad8'}) == 'xcd'
        for k in ('upper', 'out'):
            for p in ('pad1', 'off1'):
                assert f(d, u, 4, 1024, 128, places={k: p}) == 'generic'
        assert f(d, u, 4, 1024, 128, places={'tab': 'off1'}) == 'generic'
    # LDS-resident: both instantiations, the largest window, just past it, B > row chunks
    g = lambda B, Tl, D, **k: f('bf16', 'bf16', B, Tl, D, xoff=k.pop('xoff', 3), **k)   # noqa: E731
    nrt = lambda Tl: -(-Tl // 512)                                      # noqa: E731
    assert g(4, 1024, 16) == 'lds' and g(4, 1024, 48, xoff=0) == 'lds' and nrt(1024) == 2
    assert g(4, 1025, 32) == 'lds' and nrt(1025) == 3
    assert g(3, 2028, 32, xoff=0) == 'lds' and g(3, 2032, 32) == 'generic'
    assert (2028 + 15 + 4 + 15) & ~15 <= 2048 < (2032 + 15 + 4 + 15) & ~15
    assert g(300, 14, 16, xoff=0) == 'lds' and 300 > 256 // (16 // 16)
    assert g(4, 1024, 48, env={'SRNN_L1_LDS': '0'}) == 'generic'
    assert g(4, 1024, 16, Q=64) == 'generic' and g(4, 1024, 24) == 'generic'
    assert g(4, 1023, 16) == 'generic'
    assert g(4, 1024, 48, places={'upper': 'pad8'}) == 'lds'
    assert g(4, 1024, 48, places={'out': 'pad8'}) == 'lds'
    for k in ('upper', 'out'):
        for p in ('pad1', 'off1'):
            assert g(4, 1024, 48, places={k: p}) == 'generic'
    assert g(4, 1024, 48, places={'tab': 'off1'}) == 'generic'
    # the bits variant: every LDS shape, one XCD and one generic case, both layouts, ldb > D / 16
    routes = {(C.l1_route(c), c.bits) for c in T.L1_BITS}
    assert routes >= {(k, b) for k in ('lds', 'xcd', 'generic') for b in ('row', 'grouped')}
    assert all(c.D % 16 == 0 for c in T.L1_BITS)
    assert {(c.B, c.Tl, c.D) for c in T.L1_BITS if c.bits == 'row'} >= set(T._LDS_SHAPES)
    t = C.build_l1(T.L1_BITS[0])
    assert t.w['bits'].ld > t.case.D // 16
    # every dtype pair on every route it can take
    assert {(c.dtype, c.udtype) for c in T.L1_GENERIC} == set(T.DTU)
    assert {(c.dtype, c.udtype) for c in T.L1_XCD if C.l1_route(c) == 'xcd'} >= {
        ('f32', 'f32'), ('bf16', 'f32')}


def test_dtab_tables_cover_the_dispatch():
    r = C.dtab_route
    assert [r(c) for c in T.DTAB_PACKED if c.pad != 4] == ['packed'] * (len(T.DTAB_PACKED) - 1)
    assert [r(c) for c in T.DTAB_PACKED if c.pad == 4] == ['direct']
    pk = [c for c in T.DTAB_PACKED if r(c) == 'packed']
    assert {dict(c.env).get('SRNN_DTAB_PD') for c in pk} >= {None, '1', '2', '4'}
    assert {c.blk for c in pk} == {False, True} == {c.amax for c in pk}
    assert any(dict(c.env).get('SRNN_DTAB_X8') == '0' for c in pk) and any(c.pad == 8 for c in pk)
    assert {c.dist for c in pk} >= {'uniform', 'runs', 'skew'}
    assert {(c.B, c.Tl) for c in pk} >= {(3, 37), (2, 115), (5, 70), (1, 16)}
    assert set(map(r, T.DTAB_DIRECT)) == {'direct'} and set(map(r, T.DTAB_POSWS)) == {'posws'}
    assert {(c.dtype, c.out) for c in T.DTAB_DIRECT} == {(a, b) for a in ('f32', 'bf16')
                                                         for b in ('f32', 'bf16')}
    assert any(dict(c.env).get('SRNN_DTAB_PACK') == '0' and c.D == 768 for c in T.DTAB_DIRECT)
    assert any(c.D % 8 and c.dtype == c.out == 'bf16' for c in T.DTAB_DIRECT)
    assert {c.D for c in T.DTAB_POSWS} >= {8, 72, 764} and -(-764 // 4) < 192 <= -(-768 // 4)
    assert any(c.B == 40 and c.D == 8 for c in T.DTAB_POSWS)            # 40 row blocks of 1
    assert {r(c) for c in T.DTAB_GENERIC} == {'generic4', 'generic2'}
    assert {(c.FS0, c.Q) for c in T.DTAB_GENERIC} >= {(f, q) for f in (4, 20, 32) for q in (64, 256)}
    assert any(c.FS0 == 16 and dict(c.env).get('SRNN_DTAB_POS') == '0' for c in T.DTAB_GENERIC)
    assert [r(c) for c in T.DTAB_BUDGET] == ['posws', 'generic4'] * 2
    assert C.pos_lds_bytes(256, 1984) <= C.KIB160 < C.pos_lds_bytes(256, 2000)
    assert set(map(r, T.DTAB_EMPTY)) == {'empty'}
    assert sorted(c.entry for c in T.DTAB_FORWARD) == [1, 1, 2, 2, 3]
    for c in T.DTAB_EMPTY:
        t = C.build_dtab(c)
        assert not t.colsum_done and int(t.want['dtab'].abs().max()) == 0


def test_other_tables_cover_their_conditions():
    served = [c for c in T.OUT_BWD if C.out_bwd_served(c)]
    assert {(c.M, c.D, c.ranges) for c in served} >= {
        (256, 128, 0), (256, 128, 1), (1280, 384, 0), (1280, 384, 3), (8192, 1024, 0),
        (16384, 256, 0), (16384, 256, 2)}
    declined = [c for c in T.OUT_BWD if not C.out_bwd_served(c)]
    assert {(c.M, c.D) for c in declined if not c.off1} == {(128, 128), (384, 128), (256, 100)}
    assert {c.off1 for c in declined} >= {'dz', 'da2'}
    bwd = [c for c in T.NLL if c.op == 'bwd']
    assert {C.nll_bwd_route(c) for c in bwd} == {'q256', 'generic'}
    assert {(c.Q, c.place) for c in bwd if C.nll_bwd_route(c) == 'generic'} == {
        (256, 'pad1'), (256, 'off1'), (64, 'tight')}
    for op in ('bwd', 'fwd'):
        assert {c.B * c.Tl for c in T.NLL if c.op == op} == {1, 3, 4, 5, 37}
    assert {c.gmul for c in bwd} == {False, True} and all(c.ldt_extra > 0 for c in T.NLL)
    seen = set()
    for c in T.NLL:
        if c.Q == 256:
            seen |= set(C.build_nll(c).values['target'].tolist())
    assert seen >= set(C.NLL_TARGETS)
    ops = {c.op for c in T.GLUE}
    assert ops == {'srnn_gather_rows', 'srnn_scatter_add_rows', 'srnn_index_add_rows',
                   'srnn_add_bcast_rows', 'srnn_axpby', 'srnn_segsum', 'srnn_colsum',
                   'srnn_copy2d', 'srnn_permute3', 'srnn_pack_grads', 'srnn_cast_multi'}
    for op in ops - {'srnn_permute3', 'srnn_pack_grads', 'srnn_cast_multi'}:
        assert {(c.rows, c.cols) for c in T.GLUE if c.op == op} >= set(C.GLUE_SHAPES), op
    assert any(r > 65536 for r, _ in C.GLUE_SHAPES) and (0, 8) in C.GLUE_SHAPES
    assert {c.perm for c in T.GLUE if c.op == 'srnn_permute3' and c.out == 'bf16'} == set(T._PERMS)
    assert {c.perm for c in T.GLUE if c.op == 'srnn_permute3' and c.accumulate} == set(T._PERMS)
    cs = [c for c in T.GLUE if c.op == 'srnn_colsum']
    assert {c.src for c in cs} == {'f32', 'bf16'} and {c.accumulate for c in cs} == {False, True}
    assert {c.place for c in cs} >= {'pad1', 'pad8', 'off1'} and any(c.alpha != 1 for c in cs)
    assert any(c.alias for c in T.GLUE if c.op == 'srnn_axpby')
    # duplicate and absent indices
    t = C.build_glue([c for c in T.GLUE if c.op == 'srnn_scatter_add_rows' and c.rows == 37][0])
    n = torch.bincount(t.values['idx'], minlength=t.w['table'].rows)
    assert int(n.max()) > 1 and int(n.min()) == 0
    # the buckets: > 64 tensors, empty ones, NULL sources, 64-aligned offsets with gaps
    t = C.build_glue([c for c in T.GLUE if c.op == 'srnn_pack_grads'][0])
    assert len(t.sizes) > 64 and 0 in t.sizes and any(t.null) and all(o % 64 == 0 for o in t.offs)
    assert any(b - a > -(-n // 64) * 64 for a, b, n in zip(t.offs, t.offs[1:], t.sizes))
    assert len([n for n in t.sizes if n]) > 64                          # a second launch
