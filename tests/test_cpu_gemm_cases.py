"""The exact-arithmetic GEMM cases proved on the CPU (no GPU): every case of the conformance
sweep's table satisfies the exactness precondition, a float32 evaluation of it equals the
float64 reference bit for bit (so a mismatch on the GPU is the kernel's, not the method's),
the placements give the alignments they claim, the checker finds a changed output element
and a changed canary where they are, and the table covers every backend and layout."""
import pytest
import torch

import gemm_cases as G
import test_gpu_gemm_conformance as T


@pytest.mark.parametrize('name', list(T.TABLES))
def test_every_case_is_exact_in_float32(name):
    """build() asserts |alpha| |A| |B| + |beta Cin| + |bias| < 2^20 elementwise; the float32
    evaluation from the placed operands (cast to the case's dtypes and read back out of their
    windows) is the float64 reference exactly, and written into C it satisfies the checker."""
    for c in T.TABLES[name]:
        t = G.build(c)
        v = G.evaluate_f32(t)
        assert v.dtype == torch.float32 and torch.equal(v.double() + 0.0, t.ref + 0.0), c.id
        assert G.check(t) is None, c.id
        assert not G.untouched(t) or c.M * c.N == 0


def test_ids_are_unique():
    ids = [c.id for c in T.ALL_CASES]
    assert len(set(ids)) == len(ids)


def test_recipe_tests_the_rounding_mode():
    """At K = 8192 the values stay exact in fp32 while a good share of them needs rounding to
    bf16 and some are exact ties, so truncation or round-half-up on a bf16 store cannot pass."""
    c = G.case(-1, 'bf16', 'bf16', 'NT', 256, 256, 8192, 'tight', 'epi')
    t = G.build(c)
    assert torch.equal(G.evaluate_f32(t).double(), t.ref)
    assert float(t.ref.abs().max()) < 9 * 8192 * 1.5 + 16
    r32 = t.ref.float()
    bits = r32.view(torch.int32)
    inexact = (bits & 0xffff) != 0
    ties = (bits & 0xffff) == 0x8000
    assert float(inexact.float().mean()) > 0.2
    assert float(ties.float().mean()) > 0.01
    # a truncating store differs from the expected bits
    trunc = (bits & ~0xffff).view(torch.float32).to(torch.bfloat16)
    assert not torch.equal(trunc.view(torch.int16), r32.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('place', list(G.PLACEMENTS))
def test_placements_give_their_alignment(dtype, place):
    es = 4 if dtype == torch.float32 else 2
    w = G.Window(dtype, 5, 24, place, 'cpu', batch=2, extra=16)
    pad, off = G.PLACEMENTS[place]
    assert w.ld == 24 + pad and w.stride == 5 * w.ld + 16
    assert w.misalignment() == off * es
    assert w.view().stride(0) == w.ld and w.view().shape == (5, 24)
    if place in ('tight', 'pad8'):
        assert w.misalignment() == 0 and w.ld % (16 // es) == 0      # vector paths eligible
    if place == 'pad1':
        assert w.ld % 2 == 1                                        # no vector path may run
    # guard rows before and after, and everything but the windows is canary
    assert w.front >= G.GUARD_ROWS * w.ld
    assert w.buf.numel() - (w.front + w.stride + 5 * w.ld) >= G.GUARD_ROWS * w.ld
    assert w.outside_ok() and w.index.numel() == 2 * 5 * 24
    assert bool(torch.isnan(w.buf.float()).all())
    vals = torch.arange(2 * 5 * 24).view(2, 5, 24) % 7
    w.fill(vals)
    assert torch.equal(w.read().long(), vals) and w.outside_ok()
    assert w.buf[w.front + w.stride + 3 * w.ld + 2] == vals[1, 3, 2]


def test_beta_zero_leaves_cin_a_canary():
    t = G.build(G.case(1, 'f32', 'f32', 'NT', 33, 17, 5, 'pad1', 'beta0'))
    assert bool(torch.isnan(t.w['Cin'].buf).all())


def _solved(c):
    t = G.build(c)
    G.evaluate_f32(t)
    assert G.check(t) is None
    return t


@pytest.mark.parametrize('out', ['f32', 'bf16'])
def test_checker_reports_a_changed_output_element(out):
    t = _solved(G.case(1, 'bf16', out, 'NT', 37, 53, 29, 'pad1', 'full', batch=2))
    w = t.w['C']
    e = w.front + w.stride + 11 * w.ld + 7
    G._ints(w.buf)[e] ^= 1                                          # one ulp, one element
    r = G.check(t)
    assert 'inside the C window: 1 of %d elements differ' % (2 * 37 * 53) in r
    assert '(batch 1, row 11, col 7)' in r and 'outside' not in r


def test_checker_reports_a_changed_canary():
    t = _solved(G.case(1, 'bf16', 'bf16', 'NT', 37, 53, 29, 'pad1', 'full'))
    w = t.w['C']
    e = w.front + 4 * w.ld + 53                                     # row 4's padding element
    w.buf.view(torch.uint8)[2 * e] ^= 0x10                          # one byte of a canary
    r = G.check(t)
    assert 'outside the C window: 1 canary elements overwritten' in r
    assert 'row 4, col 53' in r and 'inside' not in r
    # before the window, and a written input
    t = _solved(G.case(1, 'f32', 'f32', 'NN', 37, 53, 29, 'off1', 'full'))
    t.w['C'].buf[t.w['C'].front - 1] = 0.0
    t.w['mask'].buf[0] = 1.0
    r = G.check(t)
    assert 'before the first window' in r and 'input buffer mask was written' in r


def test_checker_sees_a_write_by_a_refused_call():
    t = G.build(G.case(5, 'f32', 'f32', 'NT', 16, 16, 8, 'tight', 'plain', 'refuses'))
    assert G.untouched(t)
    t.w['C'].buf[t.w['C'].front] = 0.0
    assert not G.untouched(t)


def test_bits_layout():
    pos = torch.zeros(2, 40, dtype=torch.bool)
    pos[0, 0] = pos[0, 17] = pos[1, 15] = pos[1, 39] = True
    w = G.pack_bits(pos).view(2, 3)
    assert w.tolist() == [[1, 2, 0], [-32768, 0, 128]]


# the layouts each backend serves, from its eligibility tests
SUPPORTED = {0: ('NN', 'NT', 'TN', 'TT'), 1: ('NN', 'NT', 'TN', 'TT'), 2: ('NN', 'NT', 'TN', 'TT'),
             3: ('NN', 'NT', 'TN', 'TT'), 4: ('NT',), 5: ('NN', 'NT', 'TN', 'TT'),
             6: ('NN', 'TN', 'NT')}


def test_table_covers_every_backend():
    takes = [c for c in T.ALL_CASES if c.expect == 'takes']
    for code, layouts in SUPPORTED.items():
        mine = [c for c in takes if c.tile == code]
        for l in layouts:
            assert any(c.layout == l for c in mine), (code, l)
        # a padded and a misaligned placement each
        assert any('pad8' in (c.place,) + tuple(p for _, p in c.places) for c in mine), code
        assert any(p in (c.place,) + tuple(q for _, q in c.places) for c in mine
                   for p in ('pad1', 'off1')), code
        if code >= 3:
            assert any(c.tile == code and c.expect == 'refuses' for c in T.ALL_CASES), code
    # hipBLASLt is reached unforced: every layout, both outputs, counted
    lt = [c for c in takes if c.blaslt == 1]
    assert {(c.layout, c.out) for c in lt} >= {(l, o) for l in SUPPORTED[0] for o in ('f32', 'bf16')}
    assert any(c.place == 'pad8' for c in lt) and any(c.batch > 1 and c.sc_extra for c in lt)
    # no odd or misaligned operand goes to a shape the library takes, unless counted as + 0
    for c in T.ALL_CASES:
        odd = {c.place} | {p for _, p in c.places}
        wide = c.dtype == 'bf16' and c.M * c.N * c.batch >= 1 << 20 and 256 <= c.K <= 4096
        if c.tile < 0 and wide and odd & {'pad1', 'off1'}:
            assert c.blaslt == 0, c.id
    # one split-K path per output mode for the ring and the 256-tile kernels
    for code, k in ((3, 1024), (5, 2048)):
        sk = [c for c in takes if c.tile == code and c.K == k and c.epi == 'plain']
        assert any(not c.env and not c.places for c in sk)                       # partials
        assert any(c.env and not c.places for c in sk)                           # memset
        assert any(c.env and dict(c.places).get('C') == 'pad8' for c in sk)      # 2-D memset
