"""Exact GEMM conformance sweep: every backend of the router (csrc/gemm.hip), every layout,
padded and misaligned placements, every epilogue -- with zero tolerance.

gemm_cases.py explains the method: small-integer operands and dyadic epilogue constants make
every accumulation order give the same fp32 bits, so an fp32 output must be bit-equal to the
float64 reference and a bf16 output to its round-to-nearest-even; every operand is a window
in a canary-filled buffer, so stray reads poison the result and stray writes show.

Each row of the tables below names the forced tile code (-1: the router chooses), the input
and output dtype, the layout, the shape, the placement, the epilogue and the expectation, read
from the backend's eligibility tests:
  takes    the call returns and the checker passes.  A forced code that is offered a problem
           and declines is an error in gemm_route, so a passing forced case ran on that backend.
  refuses  RuntimeError with the router's "not eligible" message of that code, and the C
           buffer is canary throughout afterwards.
tests/test_cpu_gemm_cases.py proves on the CPU that every case here is exact by itself.
"""
import dataclasses

import pytest
import torch

import gemm_cases as G
from gemm_cases import case

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LAYOUTS = ('NN', 'NT', 'TN', 'TT')
DT4 = (('f32', 'f32'), ('f32', 'bf16'), ('bf16', 'f32'), ('bf16', 'bf16'))
DT2 = (('f32', 'f32'), ('bf16', 'bf16'))
PLACES = ('tight', 'pad8', 'pad1', 'off1')
EPIS = ('plain', 'alpha', 'cbias', 'rbias', 'cin', 'relu', 'mask', 'full', 'beta0')
PART0 = {'SRNN_G3_SPLITK_PART': '0'}

# ---- the general kernel: codes 0 / 1 / 2 = the 128 / 64 / 32 tile; it takes everything, odd
# leading dimensions and misaligned bases on the scalar loads (vecA / vecB = 0)
GENERAL = (
    # every layout x dtype pair x placement at the smallest shape (edge tiles only)
    [case(2, d, o, l, 37, 53, 29, p, 'full') for l in LAYOUTS for d, o in DT4 for p in PLACES]
    # every epilogue x dtype pair over several 64-tiles with an odd leading dimension
    + [case(1, d, o, 'NT', 130, 260, 70, 'pad1', e) for e in EPIS for d, o in DT4]
    # the 128 and 64 tiles: every layout, vector-eligible padding and a misaligned base
    + [case(t, d, o, l, 130, 260, 70, p, 'fullr') for t in (0, 1) for l in LAYOUTS
       for d, o in DT2 for p in ('pad8', 'off1')]
    + [case(0, d, o, l, 130, 260, 70, 'tight', 'full') for l in LAYOUTS
       for d, o in (('f32', 'bf16'), ('bf16', 'f32'))]
    # K = 1
    + [case(t, d, o, l, 33, 17, 1, p, 'full') for t in (0, 1, 2) for l in LAYOUTS
       for d, o, p in (('f32', 'f32', 'tight'), ('bf16', 'bf16', 'off1'))]
    # K = 0: act(beta Cin + bias) where the mask allows, and zeros for the plain product
    + [case(t, d, o, l, 64, 48, 0, 'tight', e) for t in (0, 1, 2) for l in ('NN', 'TT')
       for d, o in DT2 for e in ('fullr', 'plain')]
    # the deepest reduction of the method (sums up to 1.1e5: most bf16 outputs are rounded)
    + [case(0, 'bf16', 'bf16', 'NT', 130, 260, 8192, 'tight', 'epi'),
       case(2, 'f32', 'bf16', 'TN', 37, 53, 8192, 'pad1', 'full')]
)

# ---- strided batches run on the general kernel only (forced 0 / 1 / 2 or unforced)
BATCHED = [
    case(t, d, o, l, 40, 72, 48, 'tight', e, batch=3, **kw)
    for t in (-1, 1) for d, o in DT2 for l in ('NN', 'NT')
    for e, kw in (('alpha', {}),                                        # tight strides
                  ('cbias', dict(shared='B')),                          # sB = 0
                  ('epi', {}),                                          # sCin given
                  ('epi', dict(places={'C': 'pad8'}, sc_extra=16)),     # ldc = N + 8, padded sC
                  # the mask's batch stride is sC (not M * ldmask): its rows stay N apart
                  ('full', dict(places={'C': 'pad8'}, sc_extra=16)))
]

# ---- a forced backend whose guard fails (a batch) is refused like one that declines
FORCED_GUARD = [case(t, 'bf16', 'f32', 'NT', 256, 256, 128, 'tight', 'plain', 'refuses', batch=2)
                for t in (3, 4, 5, 6)]

# ---- thin (6): small N (plain fp32 output, B stored K x N, K >= 128, M K >= 2^16) and
# small K (K <= 64, NT, column bias only, M >= 256)
THIN = (
    [case(6, d, 'f32', 'NN', 512, n, 128, p, e) for d in ('f32', 'bf16')
     for n, p, e in ((5, 'tight', 'alpha'), (5, 'pad1', 'plain'), (64, 'pad8', 'alpha'),
                     (64, 'off1', 'plain'))]
    # A stored K x M: 4 rows per lane when M % 4 == 0 and A's rows are aligned, else scalar
    + [case(6, d, 'f32', 'TN', 512, 6, 128, p, 'alpha') for d in ('f32', 'bf16')
       for p in ('tight', 'pad8', 'pad1', 'off1')]
    + [case(6, d, 'f32', 'TN', 510, 6, 129, p, 'alpha') for d in ('f32', 'bf16')
       for p in ('tight', 'pad1')]
    + [case(6, 'bf16', 'f32', 'NN', 512, 5, 128, 'tight', 'cbias', 'refuses'),
       case(6, 'bf16', 'f32', 'NT', 512, 5, 128, 'tight', 'plain', 'refuses'),
       case(6, 'bf16', 'bf16', 'NN', 512, 5, 128, 'tight', 'plain', 'refuses'),
       case(6, 'bf16', 'f32', 'NN', 512, 5, 128, 'tight', 'mask', 'refuses')]
    # small K: the 4-column kernel (N % 4 == 0, aligned C / Cin / bias) and the scalar one
    + [case(6, d, o, 'NT', m, n, k, p, 'epi') for d, o in DT4
       for m, n, k in ((256, 40, 7), (300, 700, 64), (260, 702, 33))
       for p in ('tight', 'pad8')]
    + [case(6, 'bf16', 'bf16', 'NT', 300, 700, 64, 'tight', 'epi', places={'C': 'pad1'}),
       case(6, 'f32', 'f32', 'NT', 300, 700, 64, 'tight', 'epi', places={'bias': 'off1'}),
       case(6, 'bf16', 'f32', 'NT', 300, 700, 64, 'off1', 'epi'),
       case(6, 'bf16', 'f32', 'NT', 256, 40, 7, 'pad1', 'beta0'),
       case(6, 'bf16', 'f32', 'NT', 300, 700, 64, 'tight', 'rbias', 'refuses'),
       case(6, 'bf16', 'f32', 'NT', 255, 40, 7, 'tight', 'epi', 'refuses'),
       case(6, 'bf16', 'f32', 'NN', 256, 40, 7, 'tight', 'epi', 'refuses')]
    # small N over a deep K (many k splits summed in order)
    + [case(6, 'bf16', 'f32', 'TN', 512, 6, 8192, 'tight', 'alpha'),
       case(6, 'f32', 'f32', 'NN', 512, 64, 8192, 'pad1', 'alpha')]
)

# ---- skinny (4): NT, K a multiple of 256 bytes of elements, A and B vector-eligible
_SK_REFUSED = (
    [case(4, d, o, 'NT', 67, 256, 96, 'tight', 'full', 'refuses') for d, o in DT2]
    + [case(4, 'bf16', 'f32', l, 128, 128, 128, 'tight', 'full', 'refuses')
       for l in ('NN', 'TN', 'TT')]
    + [case(4, d, o, 'NT', 67, 256, 128, 'tight', 'full', 'refuses', places={x: p})
       for d, o in DT2 for x in ('A', 'B') for p in ('pad1', 'off1')]
)
SKINNY = (
    [case(4, d, o, 'NT', m, n, k, 'tight', e) for d, o in DT4
     for m, n, k, e in ((67, 256, 128, 'full'), (128, 40, 256, 'fullr'),
                        (67, 42, 128, 'full'))]              # N % 4 != 0: the scalar epilogue
    # padded C, Cin and mask keep the 4-column epilogue; a padded A and B keep the ring
    + [case(4, d, o, 'NT', 67, 256, 128, 'pad8', e) for d, o in DT4 for e in ('full', 'epi')]
    # an odd ldc, a misaligned C / Cin / mask / bias: vecC = 0, still taken
    + [case(4, d, o, 'NT', 67, 256, 128, 'tight', 'full', places={x: p}) for d, o in DT2
       for x, p in (('C', 'pad1'), ('C', 'off1'), ('Cin', 'pad1'), ('mask', 'off1'),
                    ('bias', 'off1'))]
    + [case(4, d, o, 'NT', 67, 256, 128, 'tight', e, env={'SRNN_SKINNY_VEC': '0'})
       for d, o in DT2 for e in ('full', 'epi')]
    + [case(4, 'bf16', 'bf16', 'NT', 600, 1024, 128, 'tight', 'full'),     # 32 x 32 tiles
       case(4, 'bf16', 'f32', 'NT', 67, 256, 128, 'tight', 'beta0')]
    # all rows in one 128-row tile (64 < M <= 128, N >= 4096): 32, 48, 64 and 80 wide
    + [case(4, 'bf16', o, 'NT', m, n, 128, 'tight', e)
       for m, n in ((100, 4096), (128, 8256), (65, 12352), (128, 16400))
       for o, e in (('bf16', 'epi'), ('f32', 'full'))]
    + [case(4, 'f32', 'f32', 'NT', 100, 4096, 128, 'pad8', 'fullr'),
       case(4, 'bf16', 'bf16', 'NT', 65, 12352, 128, 'tight', 'epi', places={'C': 'pad1'}),
       case(4, 'bf16', 'bf16', 'NT', 67, 256, 8192, 'tight', 'full'),
       case(4, 'f32', 'bf16', 'NT', 128, 40, 8192, 'pad8', 'fullr')]
    + _SK_REFUSED
)

# ---- gemm2 (3): M, N multiples of 128, K of 128 bytes of elements, aligned A and B
_G2_REFUSED = [
    case(3, 'bf16', 'f32', 'NT', 130, 256, 64, 'tight', 'full', 'refuses'),
    case(3, 'bf16', 'f32', 'NT', 128, 256, 96, 'tight', 'full', 'refuses'),
    case(3, 'bf16', 'f32', 'NT', 128, 256, 64, 'tight', 'full', 'refuses', places={'A': 'off1'}),
    case(3, 'f32', 'f32', 'NN', 128, 128, 32, 'tight', 'full', 'refuses', places={'B': 'pad1'}),
]
GEMM2 = (
    [case(3, 'bf16', o, l, 128, 256, 64, 'pad8', 'full') for o in ('f32', 'bf16')
     for l in LAYOUTS]
    + [case(3, 'f32', o, l, 128, 128, 32, 'pad8', 'fullr') for o in ('f32', 'bf16')
       for l in LAYOUTS]
    + [case(3, 'bf16', 'bf16', 'NT', 256, 128, 192, 'tight', 'full', places={x: p})
       for x, p in (('C', 'pad1'), ('C', 'off1'), ('Cin', 'pad1'), ('mask', 'off1'),
                    ('bias', 'off1'))]
    + [case(3, 'bf16', 'f32', 'NN', 128, 256, 64, 'tight', 'beta0')]
    # split K (plain, fp32 out; 2 slices at bf16, 4 at fp32): partials + ordered sum ...
    + [case(3, 'bf16', 'f32', l, 128, 128, 1024, 'tight', 'plain') for l in LAYOUTS]
    + [case(3, 'f32', 'f32', 'NT', 128, 128, 1024, 'pad8', 'alpha'),
       # ... memset + atomics, 2-D memset + atomics, and atomics because ldc % 4 != 0
       case(3, 'bf16', 'f32', 'NT', 128, 128, 1024, 'tight', 'plain', env=PART0),
       case(3, 'bf16', 'f32', 'NT', 128, 128, 1024, 'tight', 'plain', env=PART0,
            places={'C': 'pad8'}),
       case(3, 'bf16', 'f32', 'NT', 128, 128, 1024, 'tight', 'plain', places={'C': 'pad1'}),
       case(3, 'bf16', 'f32', 'NT', 128, 128, 1024, 'tight', 'plain', places={'C': 'off1'}),
       case(3, 'bf16', 'bf16', 'NN', 128, 128, 8192, 'tight', 'epi'),
       case(3, 'bf16', 'f32', 'TN', 128, 128, 8192, 'tight', 'plain')]       # 16 slices
    + _G2_REFUSED
)

# ---- gemm3 (5): bf16 inputs, M, N multiples of 256, K of 32, aligned everything
_G3_REFUSED = (
    [case(5, 'f32', 'f32', 'NT', 256, 256, 32, 'tight', 'full', 'refuses'),
     case(5, 'bf16', 'f32', 'NT', 256, 256, 48, 'tight', 'full', 'refuses'),
     case(5, 'bf16', 'f32', 'NT', 256, 250, 32, 'tight', 'full', 'refuses')]
    + [case(5, 'bf16', o, 'NT', 256, 256, 64, 'tight', 'full', 'refuses', places={x: p})
       for o in ('f32', 'bf16')
       for x, p in (('C', 'pad1'), ('A', 'off1'), ('B', 'pad1'), ('Cin', 'off1'),
                    ('bias', 'off1'), ('mask', 'pad1'))]
)
GEMM3 = (
    [case(5, 'bf16', o, l, m, n, k, 'pad8', e) for o in ('f32', 'bf16') for l in LAYOUTS
     for m, n, k, e in ((256, 256, 32, 'full'), (512, 256, 96, 'fullr'), (256, 512, 64, 'full'))]
    + [case(5, 'bf16', o, 'NT', 256, 256, 64, 'tight', e) for o in ('f32', 'bf16')
       for e in ('plain', 'alpha', 'cbias', 'rbias', 'cin1', 'relu', 'mask', 'beta0')]
    # the only misplacements gemm3 accepts: a row bias (scalar loads) and an unread Cin
    + [case(5, 'bf16', o, 'NT', 256, 256, 64, 'tight', e, places={x: 'off1'})
       for o in ('f32', 'bf16') for e, x in (('rbias', 'bias'), ('beta0', 'Cin'))]
    # split K (8 slices): partials + ordered sum, memset + atomics, 2-D memset + atomics
    + [case(5, 'bf16', 'f32', l, 256, 256, 2048, 'tight', 'plain') for l in LAYOUTS]
    + [case(5, 'bf16', 'f32', 'NT', 256, 256, 2048, 'pad8', 'alpha'),
       case(5, 'bf16', 'f32', 'NT', 256, 256, 2048, 'tight', 'plain', env=PART0),
       case(5, 'bf16', 'f32', 'NN', 256, 256, 2048, 'tight', 'plain', env=PART0,
            places={'C': 'pad8'}),
       case(5, 'bf16', 'bf16', 'NT', 256, 256, 8192, 'tight', 'epi'),
       case(5, 'bf16', 'f32', 'TN', 256, 256, 8192, 'tight', 'plain')]
    + _G3_REFUSED
)

# ---- ReLU masks as bits (row-major words, rows padded): in gemm3's epilogue (forced 5) and
# through the expanded-mask / bits-after fallback at N = 40 (a partial last word per row)
BITS = [
    case(5, 'bf16', 'bf16', 'NT', 256, 256, 64, 'tight', 'alpha', bits='in'),
    case(5, 'bf16', 'bf16', 'NN', 256, 256, 32, 'pad8', 'cbrelu', bits='out'),
    case(-1, 'bf16', 'bf16', 'NT', 48, 40, 32, 'tight', 'alpha', bits='in'),
    case(-1, 'bf16', 'bf16', 'NT', 48, 40, 32, 'pad1', 'cbrelu', bits='out'),
    case(-1, 'f32', 'f32', 'NN', 48, 40, 32, 'tight', 'alpha', bits='in'),
]

# ---- the router's own choice (-1).  What a forced vector backend refuses for an odd leading
# dimension or a misaligned base falls through to a backend that serves it.  (No pad1 / off1
# placement goes to a shape hipBLASLt could take.)
AUTO = (
    [dataclasses.replace(c, tile=-1, expect='takes')
     for c in _SK_REFUSED + _G2_REFUSED + _G3_REFUSED]
    + [case(-1, 'bf16', o, 'NT', 256, 256, 0, 'tight', e) for o in ('f32', 'bf16')
       for e in ('fullr', 'plain')]
    + [case(-1, d, o, l, 130, 260, 70, p, 'full') for d, o in DT2 for l in ('NN', 'NT')
       for p in ('pad1', 'off1')]
    # a plain deep product with one 256-tile: gemm3's split K by the router's own choice
    + [case(-1, 'bf16', 'f32', l, 256, 256, 2048, p, 'plain') for l in ('NN', 'TN')
       for p in ('tight', 'pad8')]
)

# ---- hipBLASLt (unforced: bf16, beta = 0, column bias at most, >= 1 Mi outputs over
# 256 <= K <= 4096, M N K multiples of 16, leading dimensions of 8, 16-byte bases).  blaslt =
# the rise of srnn_blaslt_calls() the call must cause.
BLASLT = (
    [case(-1, 'bf16', o, l, 1024, 1024, 256, p, e, blaslt=1) for o in ('f32', 'bf16')
     for l in LAYOUTS for e in ('plain', 'alpha', 'cbias', 'cbrelu') for p in ('tight', 'pad8')]
    + [case(-1, 'bf16', 'bf16', 'NT', 1024, 1024, 1024, 'tight', 'cbrelu', blaslt=1)]
    # one operand shared by every batch (sA = 0: the folded embedding . conv table build) and
    # a padded batch stride of C
    + [case(-1, 'bf16', o, 'NT', 256, 1024, 256, 'tight', 'plain', batch=16, shared='A',
            sc_extra=16, blaslt=1) for o in ('f32', 'bf16')]
    # what the library path does not serve stays exact on the project's kernels
    + [case(-1, 'bf16', o, 'NT', 1024, 1024, 256, 'tight', e, blaslt=0) for o in ('f32', 'bf16')
       for e in ('rbias', 'cin', 'mask')]
    # a base pointer off a 16-byte boundary never reaches the library
    + [case(-1, 'bf16', 'bf16', 'NT', 1024, 1024, 256, 'tight', 'cbias', blaslt=0,
            places={x: 'off1'}) for x in ('A', 'B', 'C', 'bias')]
)

TABLES = dict(general=GENERAL, batched=BATCHED, forced_guard=FORCED_GUARD, thin=THIN,
              skinny=SKINNY, gemm2=GEMM2, gemm3=GEMM3, bits=BITS, auto=AUTO, blaslt=BLASLT)
ALL_CASES = [c for t in TABLES.values() for c in t]


def run_case(hip, monkeypatch, c):
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    t = G.build(c, DEV)
    a, b, kw = G.gemm_kwargs(t)
    calls = hip.lib().dll.srnn_blaslt_calls
    n0 = calls()
    if c.expect == 'refuses':
        with pytest.raises(RuntimeError, match=G.INELIGIBLE[c.tile]):
            hip.gemm(a, b, **kw)
        torch.cuda.synchronize()
        assert G.untouched(t), '%s: a refused call wrote to C' % c.id
        assert all(x.unchanged() for k, x in t.w.items() if k not in ('C', 'mbo'))
        return
    hip.gemm(a, b, **kw)
    torch.cuda.synchronize()
    if c.blaslt is not None:
        assert calls() - n0 == c.blaslt, '%s: hipBLASLt calls rose by %d' % (c.id, calls() - n0)
    report = G.check(t)
    assert report is None, report


def _params(name):
    return pytest.mark.parametrize('c', TABLES[name], ids=[c.id for c in TABLES[name]])


@_params('general')
def test_general(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('batched')
def test_batched(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('forced_guard')
def test_forced_guard(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('thin')
def test_thin(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('skinny')
def test_skinny(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('gemm2')
def test_gemm2(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('gemm3')
def test_gemm3(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('bits')
def test_bits(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('auto')
def test_auto(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('blaslt')
def test_blaslt(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)
