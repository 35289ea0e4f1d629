"""Exact and step-local conformance sweep for the GRU kernels: every back end of the recurrence
(the XCD sweeps, the seq sweeps, the per-step cells, the layer entry under each plan), every
kernel the dispatchers select, padded / time-major / offset operands -- no measured tolerance.

gru_cases.py explains the three methods (A: exact forward at saturation, B: step-local
forward with derived bounds, C: exact and step-local backward) and the placement: every
operand is a window in a canary-filled buffer, outputs start as canary and work areas as 7s.

Each row names the direction, the back end, the method, the dtype, (B, D, Fr), the layout and
the switches.  `takes`: the call returns, no persistent-sweep error word is up, and the checker
passes.  `refuses`: RuntimeError with the back end's message and every output still canary.
tests/test_cpu_gru_cases.py proves every exact case exact by itself, that the tables lie on
both sides of every dispatcher condition, and that the checker catches the listed defects.
The XCD tables are laid out for a device of gru_cases.NCU compute units.
"""
import pytest
import torch

import gru_cases as G
from gru_cases import case

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FLAYOUTS = ('pad', 'tm', 'wide', 'off')
PK0, BATCH0 = {'SRNN_GX_PK': '0'}, {'SRNN_GX_BATCH': '0'}
DC0, LOCAL0 = {'SRNN_GX_DC': '0'}, {'SRNN_GEN_LOCAL': '0'}


def rows_for(D, mt):
    """A batch with a row tail whose one launch runs `mt` tiles per group (gx_layout: the
    groups of a launch are NCU / (D / 32) at most, 16 rows per tile)."""
    gmax = G.NCU // (D // 32)
    return 20 if mt == 1 else 16 * (mt // 2) * gmax + 10


# ---- the XCD sweeps, forward: D in {256, 512, 768, 1024}; D = 768 is the runtime-D form with
# cdiv(NU, NW) = 3 (ui = 2), D = 1024 the compile-time form unless SRNN_GX_DC=0
XCD_FWD = (
    [case('fwd', 'xcd2', m, 'bf16', 20, D, 3) for D in (256, 512, 768, 1024) for m in 'AB']
    + [case('fwd', 'xcd2', m, 'bf16', rows_for(D, mt), D, 2, lay)
       for D in (768, 256) for mt, lay in ((2, 'pad'), (4, 'tm')) for m in 'AB']
    + [case('fwd', 'xcd2', 'A', 'bf16', 20, 768, 3, lay) for lay in FLAYOUTS]
    + [case('fwd', 'xcd', 'A', 'bf16', 20, 256, 3, 'pad'),               # no hprev_lp
       case('fwd', 'xcd2', 'A', 'bf16', 20, 1024, 3, 'off', env=DC0),
       case('fwd', 'xcd2', 'B', 'bf16', 20, 1024, 3, env=DC0),
       case('fwd', 'xcd2', 'A', 'bf16', rows_for(1024, 2), 1024, 2, 'wide'),
       case('fwd', 'xcd2', 'A', 'bf16', 20, 512, 3, 'pad', env=LOCAL0),
       case('fwd', 'xcd2', 'A', 'bf16', 20, 256, 1, 'off')]
    # B = 1 and the edges of the 16-row tile (fewer rows per group than 16: RV < 16)
    + [case('fwd', 'xcd2', 'A', 'bf16', B, 256, 3, 'tm') for B in (1, 15, 16, 17, 129)]
    # full tiles (16 valid rows in every group): the training shape and 32 groups of D = 256
    + [case('fwd', 'xcd2', 'A', 'bf16', 128, 1024, 2), case('fwd', 'xcd2', 'A', 'bf16', 512, 256, 2)]
    + [case('fwd', 'xcd2', 'A', 'bf16', 20, 256, 2, variant='wmis', expect='refuses')]
)

# ---- the XCD sweeps, backward: the packed kernels (per tile and batched), the unpacked ones
# (SRNN_GX_PK=0; full == false at D = 768 only), MT = 1 / 2 / 4
XCD_BWD = (
    [case('bwd', 'xcd2', m, 'bf16', 20, D, 2, env=e)
     for D in (256, 512, 768, 1024) for m in ('C', 'Crne') for e in ({}, PK0)]
    + [case('bwd', 'xcd2', 'Cloc', 'bf16', 20, D, Fr, env=e)
       for D, Fr in ((256, 5), (512, 3), (768, 3), (1024, 3)) for e in ({}, PK0)]
    + [case('bwd', 'xcd2', 'C', 'bf16', rows_for(D, mt), D, 2, lay, env=e)
       for D in (768, 256) for mt, lay in ((2, 'pad'), (4, 'tm')) for e in ({}, BATCH0, PK0)]
    + [case('bwd', 'xcd2', m, 'bf16', rows_for(768, 2), 768, Fr, 'off', env=e)
       for m, Fr in (('Crne', 2), ('Cloc', 3)) for e in ({}, BATCH0, PK0)]
    + [case('bwd', 'xcd2', 'C', 'bf16', 20, 768, 2, lay, env=e) for lay in FLAYOUTS
       for e in ({}, PK0)]
    + [case('bwd', 'xcd', 'C', 'bf16', 20, 256, 2, 'pad'),               # no dgi_lp / bsum
       case('bwd', 'xcd', 'C', 'bf16', 20, 256, 2, 'pad', env=PK0),
       case('bwd', 'xcd2', 'C', 'bf16', 20, 512, 2, 'pad', env=LOCAL0),
       case('bwd', 'xcd2', 'C', 'bf16', 20, 256, 1, 'off'),
       case('bwd', 'xcd2', 'C', 'bf16', 20, 256, 1, 'off', env=PK0)]
    + [case('bwd', 'xcd2', 'C', 'bf16', B, 256, 2, 'tm') for B in (1, 15, 16, 17, 129)]
    + [case('bwd', 'xcd2', 'C', 'bf16', B, D, 2, env=e) for B, D in ((128, 1024), (512, 256))
       for e in ({}, PK0)]
    + [case('bwd', 'xcd2', 'C', 'bf16', 20, 256, 2, variant='wmis', expect='refuses')]
)

# ---- the seq sweeps: D in {128, 384} (the XCD sweeps decline D % 256 != 0), B around the
# 32-row tile.  out_lp / dgh_lp rows are handed over as 16-byte pieces: ldo, so, ldd, sd are
# multiples of 8 in every layout but 'odd', which is refused
SEQ_FWD = (
    [case('fwd', 'seq', 'A', 'bf16', B, D, 3) for D in (128, 384) for B in (1, 31, 32, 33, 40)]
    + [case('fwd', 'seq', 'B', 'bf16', 33, D, 3) for D in (128, 384)]
    + [case('fwd', 'seq', m, 'bf16', 33, 128, 3, lay) for lay in FLAYOUTS for m in 'AB']
    + [case('fwd', 'seq', 'A', 'bf16', 33, 384, 1, 'pad'),
       case('fwd', 'seq', 'A', 'bf16', 33, 128, 2, 'odd', expect='refuses'),
       case('fwd', 'seq', 'A', 'bf16', 33, 128, 2, variant='wmis', expect='refuses')]
)
SEQ_BWD = (
    [case('bwd', 'seq', 'C', 'bf16', B, D, 2) for D in (128, 384) for B in (1, 31, 32, 33, 40)]
    + [case('bwd', 'seq', m, 'bf16', 33, D, Fr) for D in (128, 384)
       for m, Fr in (('Crne', 2), ('Cloc', 3), ('Cloc', 5))]
    + [case('bwd', 'seq', m, 'bf16', 33, 128, Fr, lay) for lay in FLAYOUTS
       for m, Fr in (('C', 2), ('Cloc', 3))]
    + [case('bwd', 'seq', 'C', 'bf16', 33, 384, 1, 'pad'),
       case('bwd', 'seq', 'C', 'bf16', 33, 128, 2, 'odd', expect='refuses'),
       case('bwd', 'seq', 'C', 'bf16', 33, 128, 2, variant='wmis', expect='refuses')]
)

# ---- the cells, one launch per step: D = 48 / 80 take the plain kernels, D = 256 the ring
# kernels unless an operand fails the 16-byte test (an odd pitch or offset of h / dgh_next,
# a misaligned weight), which is the other side of launch_cell's / launch_bwd's condition
STEPS_FWD = (
    [case('fwd', 'steps', 'A', d, B, D, 3) for d in ('bf16', 'f32') for D in (48, 80, 256)
     for B in (1, 15, 16, 17, 33)]
    + [case('fwd', 'steps', 'A', d, 17, D, Fr, 'pad') for d in ('bf16', 'f32')
       for D in (48, 80, 256) for Fr in (1, 2)]
    + [case('fwd', 'steps', m, d, 33, D, 3, lay) for d in ('bf16', 'f32') for D in (48, 256)
       for lay in ('tm', 'wide', 'off') for m in 'AB']
    + [case('fwd', 'steps', 'B', d, 33, D, 3) for d in ('bf16', 'f32') for D in (48, 80, 256)]
    + [case('fwd', 'steps', m, d, 17, D, 2, lay, variant='x') for d in ('bf16', 'f32')
       for D, lay in ((48, 'pad'), (256, 'dense'), (256, 'off')) for m in 'AB']
    + [case('fwd', 'steps', 'A', d, 17, 256, 2, variant='wmis') for d in ('bf16', 'f32')]
)
STEPS_BWD = (
    [case('bwd', 'steps', 'C', d, B, D, 2, variant='both') for d in ('bf16', 'f32')
     for D in (48, 80, 256) for B in (1, 15, 16, 17, 33)]
    + [case('bwd', 'steps', 'C', d, 17, D, 1, 'pad', variant='both') for d in ('bf16', 'f32')
       for D in (48, 256)]
    + [case('bwd', 'steps', m, d, 33, D, Fr, lay, variant='both') for d in ('bf16', 'f32')
       for D in (48, 256) for lay in ('pad', 'tm', 'wide', 'off')
       for m, Fr in (('C', 2), ('Cloc', 3))]
    + [case('bwd', 'steps', m, d, 33, D, Fr, variant=v) for d in ('bf16', 'f32')
       for D, v in ((48, 'w'), (256, 'w'), (256, 'wt'), (256, 'wmis'), (80, 'both'))
       for m, Fr in (('Crne', 2), ('Cloc', 3))]
    + [case('bwd', 'steps', 'C', d, 17, 48, 2, variant='wt', expect='refuses')
       for d in ('bf16', 'f32')]
)

# ---- the layer entry under each plan; a device shared 8 ways runs 80 rows of D = 1024 as
# launches of 64 + 16 rows over GruLayerFwd / GruLayerBwd::rows() with padded and time-major
# strides
_LAYER = (('xcd', 'bf16', 20, 256), ('seq', 'bf16', 40, 128), ('steps', 'bf16', 5, 256),
          ('steps', 'f32', 5, 48), ('steps', 'f32', 5, 256))
LAYER_FWD = (
    [case('fwd', 'layer', m, d, B, D, 3, lay, plan=pl) for pl, d, B, D in _LAYER
     for lay in ('dense', 'pad', 'tm') for m in 'AB']
    + [case('fwd', 'layer', 'A', 'bf16', 80, 1024, 2, lay, plan='xcd', share=8)
       for lay in ('pad', 'tm')]
    + [case('fwd', 'layer', 'A', 'bf16', 40, 128, 2, 'odd', plan='seq', expect='refuses')]
)
LAYER_BWD = (
    [case('bwd', 'layer', m, d, B, D, Fr, lay, plan=pl) for pl, d, B, D in _LAYER
     for lay in ('dense', 'pad', 'tm') for m, Fr in (('C', 2), ('Cloc', 3))]
    + [case('bwd', 'layer', 'Crne', 'bf16', 80, 1024, 2, lay, plan='xcd', share=8)
       for lay in ('pad', 'tm')]
    + [case('bwd', 'layer', 'C', 'bf16', 40, 128, 2, 'odd', plan='seq', expect='refuses')]
)

TABLES = {'xcd_fwd': XCD_FWD, 'xcd_bwd': XCD_BWD, 'seq_fwd': SEQ_FWD, 'seq_bwd': SEQ_BWD,
          'steps_fwd': STEPS_FWD, 'steps_bwd': STEPS_BWD, 'layer_fwd': LAYER_FWD,
          'layer_bwd': LAYER_BWD}
REFUSAL = {'odd': 'multiples of 8', 'wmis': '16-byte aligned', 'wt': 'W_hh needed'}

# case id -> the largest error of r / z / n a Method B case saw, in units of 2^-24
FN_ERR = {}


def run_case(hip, monkeypatch, c):
    for k, v in G.plan_env(c).items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    t = G.build(c, DEV)
    share = hip.lib().dll.srnn_device_share()
    try:
        if c.share != share:
            hip.set_device_share(c.share)
        if c.expect == 'refuses':
            with pytest.raises(RuntimeError, match=REFUSAL[c.variant or c.layout]):
                G.run(hip, t)
            torch.cuda.synchronize()
            assert G.untouched(t), '%s: a refused call wrote to an output' % c.id
            assert all(t.w[k].unchanged() for k in t.inputs)
            return
        works = G.run(hip, t)
        torch.cuda.synchronize()
    finally:
        if c.share != share:
            hip.set_device_share(share)
    for wk in works:
        assert hip.lib().dll.srnn_gru_xcd_error(wk.data_ptr()) == 0, c.id + ': error word'
    assert hip.lib().dll.srnn_persistent_error_take() == 0, c.id + ': a sweep gave up waiting'
    report = G.check(t)
    if 'fn_err_u' in t.stats:
        FN_ERR[c.id] = t.stats['fn_err_u']
    assert report is None, report


def _params(name):
    return pytest.mark.parametrize('c', TABLES[name], ids=[c.id for c in TABLES[name]])


def test_tables_fit_the_device():
    """The XCD tables take their batch sizes from gx_layout on NCU compute units."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == G.NCU


@_params('xcd_fwd')
def test_xcd_fwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('xcd_bwd')
def test_xcd_bwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('seq_fwd')
def test_seq_fwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('seq_bwd')
def test_seq_bwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('steps_fwd')
def test_steps_fwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('steps_bwd')
def test_steps_bwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('layer_fwd')
def test_layer_fwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


@_params('layer_bwd')
def test_layer_bwd(hip, monkeypatch, c):
    run_case(hip, monkeypatch, c)


# Method B0 is Method B with W_hh = 0: gh = b_hh exactly, so what r, z and n miss the float64
# reference by is the error of the device's expf, tanhf and divide alone
ALLOWANCE = [case('fwd', 'xcd2', 'B0', 'bf16', 64, 1024, 4), case('fwd', 'xcd2', 'B0', 'bf16', 64, 768, 4),
             case('fwd', 'seq', 'B0', 'bf16', 64, 384, 4), case('fwd', 'steps', 'B0', 'bf16', 64, 256, 4),
             case('fwd', 'steps', 'B0', 'f32', 64, 80, 4)]


@pytest.mark.parametrize('c', ALLOWANCE, ids=[c.id for c in ALLOWANCE])
def test_function_allowance(hip, monkeypatch, c):
    """Method B's one measured constant: a back end's largest error in r / z / n against the
    float64 reference (printed, in units of 2^-24) stays within half of C_FN -- C_FN is twice
    the measurement, rounded up -- and C_FN within the 8 units the method allows."""
    run_case(hip, monkeypatch, c)
    print('function error of %s, units of 2^-24: %.2f' % (c.id, FN_ERR[c.id]))
    assert G.C_FN <= 8
    assert FN_ERR[c.id] <= G.C_FN / 2
