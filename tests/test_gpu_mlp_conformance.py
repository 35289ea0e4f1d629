"""Exact conformance sweep for the sample-level MLP's kernels and the glue kernels: the L1
gather (csrc/mlp.hip), the dTab scatter (csrc/dtab.hip), the output layer's backward
(csrc/out_bwd.hip), the NLL loss head and the elementwise / layout / bucket helpers
(csrc/misc.hip) -- with zero tolerance (the Adam case alone keeps its stated one).

mlp_cases.py explains the method: integer-valued operands and dyadic constants make every
order of summation give the same bits, so an fp32 output must be bit-equal to the float64
reference and a bf16 output to its round-to-nearest-even; every operand and output is a
window in a canary-filled buffer, index streams included, so stray reads poison the result
and stray writes show.

The tables put a shape on each side of every condition of the dispatchers (l1_plan, dtab_plan,
srnn_mlp_out_bwd, srnn_nll_bwd), so whichever kernel serves a shape has to be right; the L1
and dTab cases also ask the library's plan with their real operands first and fail if the
route is not the one their table is named for.
tests/test_cpu_mlp_cases.py proves on the CPU that every case is exact by itself and that
the tables do lie on both sides of those conditions.

Not expressible through the interface, so not in the tables: a padded or odd leading dimension
of the L1 table, of dTab's output and of the output backward's operands (they have no leading
dimension argument); the table gets the misaligned base only.  dTab's da is never handed over
misaligned: its dispatcher does not look at the pointer.

Time of this file on an MI355X, as pytest reports it: 7.0 s for its 343 tests, next to 5.4 s
for the 587 of test_gpu_gemm_conformance.py in the same run (both processes together took
17.5 s of wall time, start-up included); no test of this file takes longer than 1.5 s.
"""
import ctypes

import pytest
import torch

import mlp_cases as C
from mlp_cases import GlueCase, NllCase, OutBwdCase, dcase, l1case

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTU = (('f32', 'f32'), ('bf16', 'f32'), ('bf16', 'bf16'))            # table / a1, upper
# one operand at a time (the table has no leading dimension: its base alone moves)
ONE_PLACE = ([{}] + [{k: p} for k in ('upper', 'out') for p in ('pad8', 'pad1', 'off1')]
             + [{'tab': 'off1'}])

# ---- L1 gather.  generic: anything; XCD-sliced: D % 128 == 0, >= 4096 rows, 16-byte rows and
# bases; LDS-resident: bf16 / bf16, FS0 16, Q 256, D % 16 == 0, >= 4096 rows, WP <= 2048
L1_GENERIC = (
    [l1case(d, u, B, Tl, D, FS0, Q, xoff=(0, 3)[i % 2]) for d, u in DTU
     for i, (B, Tl, D, FS0, Q) in enumerate(((2, 5, 8, 4, 16), (3, 37, 20, 20, 64),
                                             (2, 40, 72, 16, 256), (1, 1, 4, 1, 256),
                                             (2, 9, 1028, 32, 256)))]
    + [l1case(d, u, 3, 37, 24, 20, 64, places=p) for d, u in DTU for p in ONE_PLACE[1:]]
)
L1_XCD = (
    [l1case(d, u, B, Tl, D) for d, u in DTU
     for B, Tl, D in ((4, 1024, 128), (3, 1365, 128), (5, 820, 256))]
    + [l1case(d, u, 4, 1024, 128, places=p) for d, u in DTU for p in ONE_PLACE[1:]]
    + [l1case('bf16', 'f32', 4, 1024, 128, FS0=20, xoff=0),          # taps past the first 16
       l1case('f32', 'f32', 4, 1024, 128, FS0=32, Q=64)]
)
_LDS_SHAPES = ((4, 1024, 16), (4, 1024, 48), (4, 1025, 32), (3, 2028, 32), (3, 2032, 32),
               (300, 14, 16), (4, 1024, 64))
L1_LDS = (
    [l1case('bf16', 'bf16', B, Tl, D, xoff=(3, 0)[i % 2]) for i, (B, Tl, D) in enumerate(_LDS_SHAPES)]
    + [l1case('bf16', 'bf16', 4, 1024, 48, env={'SRNN_L1_LDS': '0'}),
       # the other side of Q == 256, D % 16 == 0 and rows >= 4096
       l1case('bf16', 'bf16', 4, 1024, 16, Q=64), l1case('bf16', 'bf16', 4, 1024, 24),
       l1case('bf16', 'bf16', 4, 1023, 16)]
    + [l1case('bf16', 'bf16', 4, 1024, 48, places=p) for p in ONE_PLACE[1:]]
)
L1_BITS = (
    [l1case('bf16', 'bf16', B, Tl, D, bits='row') for B, Tl, D in _LDS_SHAPES]
    + [l1case('bf16', 'bf16', B, Tl, D, FS0, bits=b) for b in ('row', 'grouped')
       for B, Tl, D, FS0 in ((4, 1024, 128, 20), (3, 37, 64, 16))]
    + [l1case('bf16', 'bf16', 4, 1024, 64, bits='grouped'),
       l1case('bf16', 'bf16', 4, 1024, 64, bits='grouped', places={'out': 'pad8'}),
       l1case('bf16', 'bf16', 4, 1024, 64, bits='row', places={'upper': 'off1'})]
)

# ---- dTab (through srnn_mlp_dtab4 unless `entry` says otherwise)
_PK = ((3, 37), (2, 115), (5, 70), (1, 16))
DTAB_PACKED = (
    [dcase('bf16', 'bf16', B, Tl, 768, dist=d) for B, Tl in _PK for d in ('uniform', 'runs', 'skew')]
    + [dcase('bf16', 'bf16', B, Tl, 768, env={'SRNN_DTAB_PD': pd}, xoff=0)
       for B, Tl in ((3, 37), (5, 70)) for pd in ('1', '2', '4')]
    + [dcase('bf16', 'bf16', 5, 70, 768, blk=True, dist='runs'),
       dcase('bf16', 'bf16', 2, 115, 768, blk=True, amax=True),
       dcase('bf16', 'bf16', 3, 37, 768, amax=True, dist='skew'),
       dcase('bf16', 'bf16', 5, 70, 768, env={'SRNN_DTAB_X8': '0'}),
       dcase('bf16', 'bf16', 2, 115, 768, env={'SRNN_DTAB_X8': '0', 'SRNN_DTAB_PD': '4'}, dist='skew'),
       dcase('bf16', 'bf16', 5, 70, 768, pad=8),
       dcase('bf16', 'bf16', 5, 70, 768, pad=4),                       # ldda % 8 != 0: falls back
       dcase('bf16', 'bf16', 2, 115, 776),                             # 194 slices: no XCD map
       # sums large enough that the bf16 store has to round, ties included
       dcase('bf16', 'bf16', 5, 300, 768, dist='few', positive=True)]
)
DTAB_DIRECT = (
    [dcase('bf16', 'bf16', 3, 37, 768, env={'SRNN_DTAB_PACK': '0'}, dist='runs')]
    + [dcase(d, o, B, Tl, 768) for d, o in (('f32', 'f32'), ('f32', 'bf16'), ('bf16', 'f32'))
       for B, Tl in ((3, 37), (5, 70))]
    + [dcase('f32', 'f32', 2, 115, 768, pad=1, xoff=0), dcase('f32', 'bf16', 1, 16, 772, dist='skew'),
       dcase('bf16', 'bf16', 3, 37, 772)]                              # D % 8 != 0: not packed
)
DTAB_POSWS = (
    [dcase(d, o, 3, 37, D) for d, o in (('f32', 'f32'), ('bf16', 'bf16')) for D in (8, 72, 764)]
    + [dcase('bf16', 'f32', 40, 9, 8, dist='runs'), dcase('f32', 'bf16', 40, 9, 8, dist='skew'),
       dcase('bf16', 'bf16', 5, 70, 764, pad=1), dcase('f32', 'f32', 3, 37, 8, Q=64)]
)
DTAB_GENERIC = (
    [dcase(d, o, 3, 37, 10, FS0, Q) for d, o in (('f32', 'f32'), ('bf16', 'bf16'))
     for FS0 in (4, 20, 32) for Q in (64, 256)]
    + [dcase('bf16', 'bf16', 3, 37, 768, env={'SRNN_DTAB_POS': '0', 'SRNN_DTAB_PACK': '0'}),
       dcase('f32', 'f32', 5, 70, 12, env={'SRNN_DTAB_POS': '0'}, dist='skew'),
       dcase('f32', 'bf16', 40, 9, 8, FS0=4, Q=64, dist='runs'),
       # every entry needs rounding to bf16 (sums of ~600 terms), many of them ties
       dcase('bf16', 'bf16', 4, 600, 8, FS0=4, Q=4, positive=True)]
)
DTAB_BUDGET = [dcase(d, o, 2, Tl, 8) for d, o in (('bf16', 'bf16'), ('f32', 'f32'))
               for Tl in (1984, 2000)]
DTAB_EMPTY = [dcase('bf16', 'bf16', 0, 37, 768), dcase('f32', 'f32', 0, 37, 8),
              dcase('bf16', 'f32', 0, 5, 10, FS0=4, Q=64)]
DTAB_FORWARD = [dcase('bf16', 'bf16', 3, 37, 768, entry=1), dcase('bf16', 'bf16', 3, 37, 768, entry=2),
                dcase('bf16', 'bf16', 3, 37, 768, entry=3, amax=True),
                dcase('f32', 'f32', 3, 37, 72, entry=1), dcase('f32', 'bf16', 3, 37, 768, entry=2)]

# ---- output layer's backward: the shapes of test_gpu_out_bwd.py, two that its contract
# (M % 256 == 0, D % 128 == 0) does not serve, D = 100 and a misaligned operand
OUT_BWD = (
    [OutBwdCase(M, D, r) for M, D, r in ((256, 128, 0), (256, 128, 1), (1280, 384, 0),
                                         (1280, 384, 3), (8192, 1024, 0), (16384, 256, 0),
                                         (16384, 256, 2), (128, 128, 0), (384, 128, 2),
                                         (256, 100, 0))]
    + [OutBwdCase(256, 128, 1, want_db=False), OutBwdCase(256, 128, 1, off1='dz'),
       OutBwdCase(1280, 384, 3, off1='da2')]
)

# ---- loss head.  rows 1, 3, 4, 5, 37 as (B, Tlen); ldt = Tlen + 3
_ROWS = ((1, 1), (3, 1), (2, 2), (1, 5), (1, 37), (37, 1))
NLL = (
    [NllCase('bwd', B, Tl, 256, 'tight', gmul=g) for B, Tl in _ROWS for g in (False, True)]
    # the generic kernel: ldd % 4 != 0, a misaligned dlogp, Q = 64
    + [NllCase('bwd', B, Tl, Q, p, gmul=(B + Tl) % 2 == 0) for B, Tl in _ROWS
       for Q, p in ((256, 'pad1'), (256, 'off1'), (64, 'tight'))]
    + [NllCase('bwd', 2, 2, 256, 'pad8')]
    + [NllCase('fwd', B, Tl, Q, p) for B, Tl in _ROWS for Q, p in ((256, 'pad1'), (64, 'tight'))]
)

# ---- glue
_S = C.GLUE_SHAPES
_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
GLUE = (
    [GlueCase('srnn_gather_rows', r, c, out=o, place=p) for r, c in _S
     for o, p in (('f32', 'pad1'), ('bf16', 'off1'))]
    + [GlueCase(op, r, c) for op in ('srnn_scatter_add_rows', 'srnn_index_add_rows',
                                     'srnn_add_bcast_rows', 'srnn_segsum') for r, c in _S]
    + [GlueCase('srnn_axpby', r, c, alpha=a, beta=b, alias=al) for r, c in _S
       for a, b, al in ((1.5, -0.5, False), (1.0, 1.0, True))]
    + [GlueCase('srnn_colsum', r, c, src=s, place=p, alpha=a, accumulate=acc) for r, c in _S
       for s, p, a, acc in (('f32', 'pad1', 1.0, False), ('bf16', 'pad8', -0.5, True),
                            ('f32', 'pad8', 0.5, True), ('bf16', 'off1', 1.0, False))]
    + [GlueCase('srnn_colsum', 300, 1100, src=s, place='pad8', alpha=0.5) for s in ('f32', 'bf16')]
    + [GlueCase('srnn_copy2d', r, c, src=s, out=o) for r, c in _S
       for s in ('f32', 'bf16') for o in ('f32', 'bf16')]
    + [GlueCase('srnn_permute3', 37, 70, d0=5, perm=p, out=o) for p in _PERMS for o in ('f32', 'bf16')]
    + [GlueCase('srnn_permute3', 37, 70, d0=5, perm=p, accumulate=True) for p in _PERMS]
    + [GlueCase('srnn_permute3', r, c, d0=d, perm=p) for d, r, c in ((1, 1, 1), (2, 3, 5), (0, 8, 3),
                                                                      (70001, 2, 3))
       for p in ((2, 1, 0), (1, 0, 2))]
    + [GlueCase('srnn_pack_grads', 90, 0, out=o) for o in ('f32', 'bf16')]
    + [GlueCase('srnn_cast_multi', 90, 0, out='bf16')]
)

TABLES = dict(l1_generic=('l1', L1_GENERIC), l1_xcd=('l1', L1_XCD), l1_lds=('l1', L1_LDS),
              l1_bits=('l1', L1_BITS), dtab_packed=('dtab', DTAB_PACKED),
              dtab_direct=('dtab', DTAB_DIRECT), dtab_posws=('dtab', DTAB_POSWS),
              dtab_generic=('dtab', DTAB_GENERIC), dtab_budget=('dtab', DTAB_BUDGET),
              dtab_empty=('dtab', DTAB_EMPTY), dtab_forward=('dtab', DTAB_FORWARD),
              out_bwd=('out_bwd', OUT_BWD), nll=('nll', NLL), glue=('glue', GLUE))
ALL_CASES = [c for _, cs in TABLES.values() for c in cs]


def _p(x):
    return x.view().data_ptr() if x is not None else None


def run_l1(hip, t):
    c, w = t.case, t.w
    x = w['x']
    # the library's own plan for these operands: the kernel the table names the case for
    plan = hip.mlp_l1_plan(w['out'].dtype, w['upper'].dtype, c.B, c.Tl, c.D, c.FS0, c.Q,
                           _p(w['tab']), _p(w['upper']), w['upper'].ld, _p(w['out']), w['out'].ld,
                           have_bits=bool(c.bits))
    if plan.route != C.l1_route(c):
        return '%s: planned %s, the table says %s' % (c.id, plan.route, C.l1_route(c))
    if c.bits:
        hip.lib().call('srnn_mlp_l1_bits', _p(w['tab']), _p(x), x.ld, x.xoff, c.B, c.Tl,
                       _p(w['upper']), w['upper'].ld, _p(w['out']), w['out'].ld, c.D, c.FS0, c.Q,
                       _p(w['bits']), w['bits'].ld if c.bits == 'row' else 0, hip.stream())
    else:
        hip.lib().call('srnn_mlp_l1', hip.dcode(w['out'].dtype), _p(w['tab']), _p(x), x.ld, x.xoff,
                       c.B, c.Tl, hip.dcode(w['upper'].dtype), _p(w['upper']), w['upper'].ld,
                       _p(w['out']), w['out'].ld, c.D, c.FS0, c.Q, hip.stream())
    torch.cuda.synchronize()
    return C.check(t)


def run_dtab(hip, t):
    c, w = t.case, t.w
    x = w['x']
    work = torch.empty(t.work_elems, device=DEV, dtype=torch.int64)     # scratch, not an operand
    done = ctypes.c_int(-1)
    # the library's own plan on this device: the route the table names the case for
    plan = hip.mlp_dtab_plan(w['da'].dtype, w['dtab'].dtype, c.B, c.Tl, c.D, c.FS0, c.Q,
                             ldda=w['da'].ld, have_amax='amax' in w, have_blk='blk' in w,
                             work_bytes=work.numel() * 8)
    route = plan.route + (str(plan.cw) if plan.route == 'generic' else '')
    if route != t.route:
        return '%s: planned %s, the table says %s' % (c.id, route, t.route)
    head = (hip.dcode(w['da'].dtype), _p(w['da']), w['da'].ld, _p(x), x.ld, x.xoff, c.B, c.Tl,
            _p(w['dtab']), hip.dcode(w['dtab'].dtype), c.D, c.FS0, c.Q, hip.ptr(work),
            work.numel() * 8)
    cs = (_p(w.get('colsum')), ctypes.byref(done))
    if c.entry == 1:
        hip.lib().call('srnn_mlp_dtab', *head, hip.stream())
    elif c.entry == 2:
        hip.lib().call('srnn_mlp_dtab2', *head, *cs, hip.stream())
    elif c.entry == 3:
        hip.lib().call('srnn_mlp_dtab3', *head, *cs, _p(w.get('amax')), hip.stream())
    else:
        hip.lib().call('srnn_mlp_dtab4', *head, *cs, _p(w.get('amax')), _p(w.get('blk')),
                       hip.stream())
    torch.cuda.synchronize()
    return C.check_dtab(t, done.value if c.entry >= 2 else 0)


def run_out_bwd(hip, t):
    c, w = t.case, t.w
    Q, served = C.OB_Q, C.out_bwd_served(c)
    shape_ok = C.out_bwd_served(OutBwdCase(c.M, c.D, c.ranges))
    R = hip.lib().dll.srnn_mlp_out_bwd_ranges(hip.BF16, c.M, c.D, Q, c.ranges)
    if (R > 0) != shape_ok:
        return '%s: srnn_mlp_out_bwd_ranges gives %d' % (c.id, R)
    taken = ctypes.c_int(-1)
    hip.lib().call('srnn_mlp_out_bwd', hip.BF16, _p(w['dz']), _p(w['a2']), _p(w['wt']), c.M, c.D,
                   Q, _p(w['da2']), _p(w['dW']), _p(w.get('db')), _p(w['csp']), R,
                   ctypes.byref(taken), hip.stream())
    torch.cuda.synchronize()
    if taken.value != int(served):
        return '%s: taken = %d' % (c.id, taken.value)
    fused = hip.mlp_out_bwd(w['dz'].view(), w['a2'].view(), w['wt'].view(), c.ranges, c.want_db)
    torch.cuda.synchronize()
    if not served:
        # declined: nothing written, and the wrapper (which allocates aligned outputs of its
        # own) sends its caller to the separate calls
        ran = fused is not None
        if ran != (shape_ok and c.off1 not in ('dz', 'a2', 'wt')):
            return '%s: the wrapper %s' % (c.id, 'ran' if ran else 'declined')
        return C.untouched(t)
    if fused is None:
        return '%s: the wrapper declined' % c.id
    for k, got in zip(('da2', 'dW', 'db', 'csp'), fused):
        if k in t.want and not torch.equal(C._ints(got.cpu() + 0.0).view(-1), t.want[k].view(-1)):
            return '%s: mlp_out_bwd()\'s %s differs from the reference' % (c.id, k)
    # the hidden-bias partials reduced as mlp_backward reduces them (srnn_colsum over csp)
    got = hip.colsum(w['csp'].view(), w['csp'].rows, c.D, lds=w['csp'].ld)
    if not torch.equal(got.cpu().double(), t.ref['db_hid']):
        return '%s: the hidden bias sums differ from the reference' % c.id
    return C.check(t)


def run_nll(hip, t):
    c, w = t.case, t.w
    tg, rows = w['target'], c.B * c.Tl
    if c.op == 'bwd':
        hip.lib().call('srnn_nll_bwd', _p(tg), tg.ld, c.Tl, rows, c.Q, _p(w['dlogp']),
                       w['dlogp'].ld, t.gscale, _p(w.get('gmul')), hip.stream())
    else:
        hip.lib().call('srnn_nll_fwd', _p(w['logp']), w['logp'].ld, _p(tg), tg.ld, c.Tl, rows,
                       _p(w['loss']), hip.stream())
    torch.cuda.synchronize()
    return C.check(t)


def _arr(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def run_glue(hip, t):
    c, w, op, s = t.case, t.w, t.case.op, hip.stream()
    call = hip.lib().call
    R, Cn = c.rows, c.cols
    if op == 'srnn_gather_rows':
        call('srnn_gather_rows', _p(w['table']), w['table'].ld, _p(w['idx']), R, Cn, _p(w['out']),
             hip.dcode(w['out'].dtype), w['out'].ld, s)
    elif op == 'srnn_scatter_add_rows':
        call('srnn_scatter_add_rows', _p(w['table']), w['table'].ld, _p(w['idx']), R, Cn,
             _p(w['src']), w['src'].ld, s)
    elif op == 'srnn_index_add_rows':
        call('srnn_index_add_rows', _p(w['table']), w['table'].ld, w['table'].rows, _p(w['idx']),
             R, Cn, _p(w['src']), w['src'].ld, s)
    elif op == 'srnn_add_bcast_rows':
        call('srnn_add_bcast_rows', _p(w['x']), _p(w['v']), R, 2, Cn, w['v'].ld, s)
    elif op == 'srnn_axpby':                    # out aliasing a, as model.py sums the biases
        call('srnn_axpby', _p(w['a' if c.alias else 'out']), _p(w['a']), _p(w['b']), c.alpha,
             c.beta, R * Cn, s)
    elif op == 'srnn_segsum':
        call('srnn_segsum', _p(w['src']), w['src'].ld, R, 3, Cn, _p(w['out']), s)
    elif op == 'srnn_colsum':
        work = torch.empty(t.work_elems, device=DEV, dtype=torch.float32)
        call('srnn_colsum', hip.dcode(w['src'].dtype), _p(w['src']), w['src'].ld, R, Cn,
             _p(w['out']), c.alpha, int(c.accumulate), hip.ptr(work), work.numel(), s)
    elif op == 'srnn_copy2d':
        call('srnn_copy2d', hip.dcode(w['src'].dtype), hip.dcode(w['out'].dtype), R, Cn,
             _p(w['src']), w['src'].ld, _p(w['out']), w['out'].ld, s)
        # the cast helper over the same values (a contiguous copy of its own)
        if R * Cn and c.src != c.out:
            got = hip.cast(w['src'].read()[0], w['out'].dtype)
            if not torch.equal(C._ints(got.cpu() + 0.0).view(-1), t.want['out'].view(-1)):
                return '%s: cast() differs from the reference' % c.id
    elif op == 'srnn_permute3':
        d = t.dims
        call('srnn_permute3', _p(w['src']), _p(w['out']), hip.dcode(w['out'].dtype), d[0], d[1],
             d[2], c.perm[0], c.perm[1], c.perm[2], int(c.accumulate), s)
    elif op == 'srnn_pack_grads':
        n = len(t.sizes)
        src = [None if t.null[i] else _p(w['src%d' % i]) for i in range(n)]
        call('srnn_pack_grads', n, _arr(src), _i64(t.sizes), _i64(t.offs),
             w['flat'].buf.data_ptr() + w['flat'].front * w['flat'].buf.element_size(),
             hip.dcode(w['flat'].dtype), s)
    elif op == 'srnn_cast_multi':
        n = len(t.sizes)
        call('srnn_cast_multi', n, _arr([_p(w['src%d' % i]) for i in range(n)]),
             _arr([_p(w['dst%d' % i]) for i in range(n)]), _i64(t.sizes), s)
    else:
        raise ValueError(op)
    torch.cuda.synchronize()
    return C.check(t)


RUNNERS = dict(l1=run_l1, dtab=run_dtab, out_bwd=run_out_bwd, nll=run_nll, glue=run_glue)


def run_case(hip, monkeypatch, name, c):
    family = TABLES[name][0]
    for k, v in getattr(c, 'env', ()):
        monkeypatch.setenv(k, v)
    t = C.FAMILIES[family][0](c, DEV)
    report = RUNNERS[family](hip, t)
    assert report is None, report


def _params(name):
    return pytest.mark.parametrize('c', TABLES[name][1], ids=[c.id for c in TABLES[name][1]])


@_params('l1_generic')
def test_l1_generic(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'l1_generic', c)


@_params('l1_xcd')
def test_l1_xcd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'l1_xcd', c)


@_params('l1_lds')
def test_l1_lds(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'l1_lds', c)


@_params('l1_bits')
def test_l1_bits(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'l1_bits', c)


@_params('dtab_packed')
def test_dtab_packed(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'dtab_packed', c)


@_params('dtab_direct')
def test_dtab_direct(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'dtab_direct', c)


@_params('dtab_posws')
def test_dtab_posws(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'dtab_posws', c)


@_params('dtab_generic')
def test_dtab_generic(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'dtab_generic', c)


@_params('dtab_budget')
def test_dtab_budget(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'dtab_budget', c)


@_params('dtab_empty')
def test_dtab_empty(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'dtab_empty', c)


@_params('dtab_forward')
def test_dtab_forward(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'dtab_forward', c)


@_params('out_bwd')
def test_out_bwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'out_bwd', c)


@_params('nll')
def test_nll(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'nll', c)


@_params('glue')
def test_glue(hip, monkeypatch, c):
    run_case(hip, monkeypatch, 'glue', c)


def test_adam_clip_multi2_bf16_gradients(hip):
    """srnn_adam_clip_multi2 (and, for the last step, srnn_adam_clip_multi3 with the step count
    on the device) over bf16 gradients with gscale = 0.5, NULL gradients (all-zero
    ones) and bf16 parameter copies, 70 ragged tensors (two launches), 3 steps, against
    torch.optim.Adam on the CPU fed clamp(gscale * float(g_bf16)) -- the tolerance of
    test_adam_clip_multi_matches_torch.  The copies are bit-equal to p.to(bfloat16) and the
    gradient buffers come back unchanged."""
    sizes = ([1, 3, 7, 64, 1000, 2049, 4096, 10007] * 9)[:70]
    n = len(sizes)
    gen = torch.Generator().manual_seed(11)
    ps = [torch.randn(k, generator=gen).to(DEV) for k in sizes]
    ms = [torch.zeros(k, device=DEV) for k in sizes]
    vs = [torch.zeros(k, device=DEV) for k in sizes]
    lps = [torch.full((k,), float('nan'), device=DEV, dtype=torch.bfloat16) for k in sizes]
    refs = [p.detach().cpu().clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam(refs, lr=1e-3)
    arr = lambda ts: _arr([None if x is None else x.data_ptr() for x in ts])   # noqa: E731
    for step in range(1, 4):
        gs = [None if (i + step) % 6 == 0 else
              (torch.randn(k, generator=gen) * 3.0).to(DEV, torch.bfloat16)
              for i, k in enumerate(sizes)]
        before = [None if g is None else g.clone() for g in gs]
        if step < 3:
            hip.lib().call('srnn_adam_clip_multi2', n, arr(ps), arr(gs), hip.BF16, 0.5, arr(ms),
                           arr(vs), arr(lps), _i64(sizes), -1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8,
                           step, hip.stream())
        else:                                   # the step count read on the device
            dstep = torch.tensor([step - 1], device=DEV, dtype=torch.int64)
            hip.lib().call('srnn_adam_clip_multi3', n, arr(ps), arr(gs), hip.BF16, 0.5, arr(ms),
                           arr(vs), arr(lps), _i64(sizes), -1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0,
                           hip.ptr(dstep), hip.stream())
        torch.cuda.synchronize()
        for r, g in zip(refs, gs):
            r.grad = torch.zeros_like(r) if g is None else (0.5 * g.float().cpu()).clamp(-1, 1)
        opt.step()
        for g, b in zip(gs, before):
            assert g is None or torch.equal(g.view(torch.int16), b.view(torch.int16))
    for p, r, lp in zip(ps, refs, lps):
        torch.testing.assert_close(p.cpu(), r.detach(), atol=1e-7, rtol=1e-6)
        assert torch.equal(lp.view(torch.int16), p.to(torch.bfloat16).view(torch.int16))
