"""Batched persistent GRU sweeps (gru_xcd.hip, MT > 1: two row tiles per phase) against the
per-tile kernels they replace (SRNN_GX_BATCH=0): same arithmetic per row, so every output is
bit-identical.  Only the reverse sweep has a batched form; the forward sweep runs the same
kernel under both settings (its outputs feed the reverse sweep and are compared all the
same)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'

# (B, D, Fr): the smallest shapes that reach each batched path (8 groups at D = 1024)
SHAPES = [
    (200, 1024, 5),     # MT = 2, 13 valid rows per tile: padding lanes
    (256, 1024, 2),     # MT = 2, full tiles, one buffer flip
    (300, 1024, 5),     # MT = 4, 10 valid rows
    (512, 1024, 3),     # MT = 4, the benchmark's layout, odd step count
    (512, 1024, 1),     # no hand-off is ever consumed in the backward
    (1024, 512, 4),     # MT = 4 at another group width, runtime-D forward kernel
]

NAMES = ('out', 'out_lp', 'gates', 'hp', 'dgh', 'dgi', 'bsum', 'ddir0')


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), device=DEV, dtype=dtype)


@pytest.mark.parametrize('B,D,Fr', SHAPES)
def test_gru_xcd_batched_bit_identical(hip, B, D, Fr, monkeypatch):
    T = torch.bfloat16
    g = torch.Generator().manual_seed(B * 3 + D + Fr)
    whh = (torch.randn(3 * D, D, generator=g) * 0.03).to(DEV, T)
    whh_t = whh.float().t().contiguous().to(T)
    bhh = (torch.randn(3 * D, generator=g) * 0.1).to(DEV)
    gi = (torch.randn(B, Fr, 3 * D, generator=g) * 0.5).to(DEV)
    h0 = (torch.randn(B, D, generator=g) * 0.5).to(DEV)
    dy = (torch.randn(B, Fr, D, generator=g) * 0.1).to(DEV)
    nf = hip.gru_xcd_work_bytes(T, B, D)
    nb = hip.gru_xcd_bwd_work_bytes(T, B, D)
    assert nf and nb

    def run(batch):
        monkeypatch.setenv('SRNN_GX_BATCH', batch)
        # outputs start as NaN and the work buffers as 7s: an unwritten element or a stale tag
        # shows
        wf = torch.full((nf,), 7, device=DEV, dtype=torch.uint8)
        wb = torch.full((nb,), 7, device=DEV, dtype=torch.uint8)
        out = _nan((B, Fr, D))
        outT = _nan((B, Fr, D), T)
        gt = _nan((B, Fr, 4 * D))
        hp = _nan((B, Fr, D), T)
        hip.lib().call('srnn_gru_xcd_fwd2', hip.BF16, B, D, Fr, hip.ptr(gi), Fr * 3 * D, 3 * D,
                       hip.ptr(h0), hip.ptr(whh), hip.ptr(bhh), hip.ptr(out), hip.ptr(outT),
                       Fr * D, D, hip.ptr(gt), Fr * 4 * D, 4 * D, hip.ptr(hp), hip.ptr(wf), nf,
                       hip.stream())
        dgh = _nan((B, Fr, 3 * D), T)
        dgi = _nan((B, Fr, 3 * D), T)
        bsum = _nan((B, 4 * D))
        ddir = _nan((B, D))
        hip.lib().call('srnn_gru_xcd_bwd2', hip.BF16, B, D, Fr, hip.ptr(dy), Fr * D, D,
                       hip.ptr(gt), Fr * 4 * D, 4 * D, hip.ptr(out), Fr * D, D, hip.ptr(h0),
                       hip.ptr(whh_t), None, hip.ptr(dgh), None, hip.ptr(dgi), hip.ptr(bsum),
                       Fr * 3 * D, 3 * D, hip.ptr(ddir), hip.ptr(wb), nb, hip.stream())
        torch.cuda.synchronize()
        assert hip.lib().dll.srnn_gru_xcd_error(hip.ptr(wf)) == 0
        assert hip.lib().dll.srnn_gru_xcd_error(hip.ptr(wb)) == 0
        return [x.cpu() for x in (out, outT, gt, hp, dgh, dgi, bsum, ddir)]

    per_tile = run('0')
    batched = run('1')
    for name, a, b in zip(NAMES, batched, per_tile):
        assert not torch.isnan(a.float()).any(), name     # (NaN != NaN: say which is unwritten)
        assert torch.equal(a, b), name
