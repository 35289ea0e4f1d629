"""The sample-level MLP's plans (csrc/mlp_plan.hpp: dtab_plan, l1_plan) through
srnn_mlp_dtab_plan_for and srnn_mlp_l1_plan_for on the loaded library.  Both are pure
functions of shapes, strides, pointer alignments and switches, so they are checked here
without a device -- against mlp_cases.dtab_route / l1_route, the independent statement of the
routes that the conformance tables are laid out with, for every case of those tables."""
import pytest

import gemm_cases as G
import mlp_cases as C
import samplernn_hip as H
import test_gpu_mlp_conformance as T

DT = G.DTYPES
BASE = 0x7f0000000000          # a 16-byte aligned address that is never dereferenced
DTAB_TABLES = [k for k, (f, _) in T.TABLES.items() if f == 'dtab']
L1_TABLES = [k for k, (f, _) in T.TABLES.items() if f == 'l1']
DTAB_CASES = [c for k in DTAB_TABLES for c in T.TABLES[k][1]]
L1_CASES = [c for k in L1_TABLES for c in T.TABLES[k][1]]
SWITCHES = ['SRNN_DTAB_' + k for k in ('PACK', 'POS', 'X8', 'BLK', 'PD')] + ['SRNN_L1_LDS']


@pytest.fixture(autouse=True)
def _switches_default(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _env(monkeypatch, c):
    for k, v in c.env:
        monkeypatch.setenv(k, v)


def dplan(c, packed_ok=1, work_bytes=None):
    """The plan of a DtabCase as run_dtab calls it: ldda = D + pad, its int64 scratch."""
    n = c.Q * c.FS0 * c.D
    return H.mlp_dtab_plan(DT[c.dtype], DT[c.out], c.B, c.Tl, c.D, c.FS0, c.Q, ldda=c.D + c.pad,
                           have_amax=c.amax, have_blk=c.blk, packed_ok=packed_ok,
                           work_bytes=(n + 64) * 8 if work_bytes is None else work_bytes)


def route_name(p):
    return p.route + (str(p.cw) if p.route == 'generic' else '')


def lplan(c):
    """The plan of an L1Case with fake operand addresses of the case's alignment."""
    es, ue = DT[c.dtype].itemsize, DT[c.udtype].itemsize
    pl = {k: G.PLACEMENTS[c.placement(k)] for k in ('tab', 'upper', 'out')}
    return H.mlp_l1_plan(DT[c.dtype], DT[c.udtype], c.B, c.Tl, c.D, c.FS0, c.Q,
                         BASE + pl['tab'][1] * es, BASE + pl['upper'][1] * ue, c.D + pl['upper'][0],
                         BASE + pl['out'][1] * es, c.D + pl['out'][0], have_bits=bool(c.bits))


@pytest.mark.parametrize('c', DTAB_CASES, ids=[c.id for c in DTAB_CASES])
def test_dtab_plan_is_the_tables_route(monkeypatch, c):
    _env(monkeypatch, c)
    p = dplan(c)
    assert route_name(p) == C.dtab_route(c)
    assert p.colsum == (p.route in ('packed', 'direct'))
    assert p.work_bytes == c.Q * c.FS0 * c.D * 8


@pytest.mark.parametrize('c', L1_CASES, ids=[c.id for c in L1_CASES])
def test_l1_plan_is_the_tables_route(monkeypatch, c):
    _env(monkeypatch, c)
    p = lplan(c)
    assert p.route == C.l1_route(c)
    assert p.bits_pass == (bool(c.bits) and p.route != 'lds')


def test_off1_addresses_are_two_or_four_bytes_past_a_boundary():
    assert G.PLACEMENTS['off1'] == (0, 1) and BASE % 16 == 0
    assert DT['bf16'].itemsize == 2 and DT['f32'].itemsize == 4


def test_without_the_device_fact_nothing_is_packed(monkeypatch):
    import dataclasses
    packed = 0
    for c in DTAB_CASES:
        with monkeypatch.context() as m:
            _env(m, c)
            p = dplan(c, packed_ok=0)
            was = C.dtab_route(c)
            off = dataclasses.replace(c, env=tuple(sorted(dict(c.env, SRNN_DTAB_PACK='0').items())))
            assert p.route != 'packed' and route_name(p) == C.dtab_route(off), c.id
            packed += was == 'packed'
    assert packed >= 20


def test_prefetch_depth(monkeypatch):
    pd = lambda B: dplan(C.dcase('bf16', 'bf16', B, 16, 768)).pd        # noqa: E731
    assert (pd(383), pd(384)) == (2, 1)
    for v, want in (('1', 1), ('2', 2), ('4', 4), ('3', 4)):
        monkeypatch.setenv('SRNN_DTAB_PD', v)
        assert (pd(383), pd(384)) == (want, want)
    monkeypatch.setenv('SRNN_DTAB_PD', '')                              # empty: as if unset
    assert (pd(383), pd(384)) == (2, 1)


def test_byte_windows_need_room_and_their_switch(monkeypatch):
    c = C.dcase('bf16', 'bf16', 5, 70, 768)
    stat = 4 * 4 + 256 * 4                                              # DtabStat
    room = (stat + 255) // 256 * 256 + c.B * ((c.Tl + 15 + 15) // 16 * 16)
    assert room == 1280 + 5 * 96
    assert dplan(c, work_bytes=room).x8 and not dplan(c, work_bytes=room - 1).x8
    assert dplan(c, work_bytes=room - 1).route == 'packed'
    assert dplan(c, work_bytes=stat).route == 'packed' and dplan(c, work_bytes=stat - 1).route == 'direct'
    monkeypatch.setenv('SRNN_DTAB_X8', '0')
    assert not dplan(c, work_bytes=room).x8
    monkeypatch.delenv('SRNN_DTAB_X8')
    assert dplan(c).x8 and not dplan(c).use_blk
    blk = C.dcase('bf16', 'bf16', 5, 70, 768, blk=True)
    assert dplan(blk).use_blk
    monkeypatch.setenv('SRNN_DTAB_BLK', '0')
    assert not dplan(blk).use_blk and dplan(blk).route == 'packed'
    monkeypatch.setenv('SRNN_DTAB_BLK', '1')
    assert dplan(blk).use_blk and not dplan(c).use_blk


def test_switches_are_read_per_call(monkeypatch):
    c = C.dcase('bf16', 'bf16', 3, 37, 768)
    assert dplan(c).route == 'packed'
    monkeypatch.setenv('SRNN_DTAB_PACK', '0')
    assert dplan(c).route == 'direct'
    monkeypatch.setenv('SRNN_DTAB_POS', '0')
    assert route_name(dplan(c)) == 'generic4'
    monkeypatch.delenv('SRNN_DTAB_PACK')
    assert dplan(c).route == 'packed'
    monkeypatch.setenv('SRNN_DTAB_PACK', '01')                          # first character '0'
    assert route_name(dplan(c)) == 'generic4'
    monkeypatch.delenv('SRNN_DTAB_PACK')
    monkeypatch.delenv('SRNN_DTAB_POS')
    g = C.l1case('bf16', 'bf16', 4, 1024, 48)
    assert lplan(g).route == 'lds'
    monkeypatch.setenv('SRNN_L1_LDS', '0')
    assert lplan(g).route == 'generic'
    monkeypatch.delenv('SRNN_L1_LDS')
    assert lplan(g).route == 'lds'


def l1(dtype='bf16', udtype='bf16', B=4, Tl=1024, D=48, FS0=16, Q=256, tab=0, upper=0, out=0,
       ldu=None, ldo=None, **kw):
    """One L1 plan around the base shape; tab / upper / out: bytes past a 16-byte boundary."""
    return H.mlp_l1_plan(DT[dtype], DT[udtype], B, Tl, D, FS0, Q, BASE + tab, BASE + upper,
                         D if ldu is None else ldu, BASE + out, D if ldo is None else ldo, **kw)


def test_l1_conditions_flip_one_at_a_time(monkeypatch):
    """Each condition of the LDS and of the XCD conjunction alone, around B = 4, Tl = 1024,
    bf16 / bf16 at D = 48 (LDS, no XCD behind it) and D = 128 (LDS, XCD behind it)."""
    assert l1().route == 'lds' and l1(D=128).route == 'lds'
    assert not l1(have_bits=True).bits_pass and l1(D=40, have_bits=True).bits_pass
    # the LDS kernel's own conditions: D = 128 falls to XCD, D = 48 to generic
    for kw in (dict(Q=64), dict(FS0=20), dict(Tl=2049, B=2), dict(dtype='f32'),
               dict(udtype='f32')):
        assert l1(D=128, **kw).route == 'xcd', kw
        assert l1(D=48, **kw).route == 'generic', kw
    assert l1(D=40).route == 'generic' and l1(D=136).route == 'generic'     # D % 16
    assert l1(D=64).route == 'lds' and l1(D=64, Q=64).route == 'generic'     # D % 128
    assert l1(D=4096 + 16).route == 'generic' and l1(D=4096).route == 'lds'  # 256 column groups
    assert l1(B=3, Tl=2029).route == 'lds' and l1(B=3, Tl=2030).route == 'generic'
    monkeypatch.setenv('SRNN_L1_LDS', '0')
    assert l1(D=128).route == 'xcd' and l1().route == 'generic'
    assert l1(D=128, have_bits=True).bits_pass
    monkeypatch.delenv('SRNN_L1_LDS')
    # what both sliced kernels need: one miss sends either shape to generic
    for kw in (dict(B=1, Tl=4095), dict(ldu=132), dict(ldo=132), dict(tab=2), dict(upper=2),
               dict(out=2), dict(tab=8), dict(upper=8), dict(out=8), dict(have_base=True)):
        for D in (48, 128):
            kw2 = {k: v - 128 + D if k in ('ldu', 'ldo') else v for k, v in kw.items()}
            assert l1(D=D, **kw2).route == 'generic', (D, kw)
    assert l1(B=1, Tl=4096, D=128, Q=64).route == 'xcd'
    assert l1(B=1, Tl=4095, D=128, Q=64).route == 'generic'
    assert l1(D=128, ldu=136, ldo=144).route == 'lds'                       # multiples of 8
    # fp32 rows: 16 bytes are 4 elements
    f = dict(dtype='f32', udtype='f32', D=128)
    assert l1(ldu=132, ldo=132, **f).route == 'xcd' and l1(ldu=130, **f).route == 'generic'
    assert l1(ldo=130, **f).route == 'generic' and l1(upper=4, **f).route == 'generic'
    # a bf16 table under an fp32 upper: ldu in 4-element steps, ldo in 8-element steps
    m = dict(dtype='bf16', udtype='f32', D=128)
    assert l1(ldu=132, **m).route == 'xcd' and l1(ldo=132, **m).route == 'generic'
    assert l1(ldo=136, **m).route == 'xcd'


def test_named_results_and_codes():
    assert H.DTAB_ROUTES == ('empty', 'generic', 'posws', 'direct', 'packed')
    assert H.L1_ROUTES == ('generic', 'xcd', 'lds')
    hdr = open(H.os.path.join(H.os.path.dirname(H.HERE), 'include', 'samplernn_hip.h')).read()
    for i, k in enumerate(H.DTAB_ROUTES):
        assert 'SRNN_DTAB_%s = %d' % (k.upper(), i) in hdr
    for i, k in enumerate(H.L1_ROUTES):
        assert 'SRNN_L1_%s = %d' % (k.upper(), i) in hdr
    for name in ('srnn_mlp_dtab_plan', 'srnn_mlp_dtab_plan_for', 'srnn_mlp_l1_plan_for'):
        assert name in H._SIGS and name in H.exported_symbols()
    # an empty call: no rows, nothing to scatter, the workspace still sized
    p = dplan(C.dcase('f32', 'f32', 0, 37, 8))
    assert p == H.DtabPlan('empty', 0, 0, False, False, False, 256 * 16 * 8 * 8)
