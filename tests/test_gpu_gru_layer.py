"""The GRU layer driver (csrc/gru_layer.hpp): srnn_gru_layer_fwd / _bwd against the forced
form of the back end the plan names -- the XCD sweeps, the gru_seq sweeps, or the loop of
per-step cell launches written out here -- on the same inputs.  The driver adds no arithmetic,
so every comparison is torch.equal.  Outputs start as NaN and work buffers as 7s: an element
the call did not write, or a work area it did not clear, shows."""
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF = torch.bfloat16


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), device=DEV, dtype=dtype)


def _work(nbytes):
    return torch.full((max(nbytes, 1),), 7, device=DEV, dtype=torch.uint8)


def _inputs(T, B, D, Fr):
    g = torch.Generator().manual_seed(B * 5 + D + Fr)
    w = torch.randn(3 * D, D, generator=g) * 0.03
    return dict(whh=w.to(DEV, T), whh_t=w.t().contiguous().to(DEV, T),
                bhh=(torch.randn(3 * D, generator=g) * 0.1).to(DEV),
                gi=(torch.randn(B, Fr, 3 * D, generator=g) * 0.5).to(DEV),
                h0=(torch.randn(B, D, generator=g) * 0.5).to(DEV),
                dy=(torch.randn(B, Fr, D, generator=g) * 0.1).to(DEV))


def _fwd_bufs(T, B, D, Fr, hprev):
    lp = T != torch.float32
    return dict(out=_nan((B, Fr, D)), out_lp=_nan((B, Fr, D), T) if lp else None,
                gates=_nan((B, Fr, 4 * D)), hprev=_nan((B, Fr, D), T) if hprev else None)


def _bwd_bufs(T, B, D, Fr, xcd):
    lp = T != torch.float32
    g3 = (B, Fr, 3 * D)
    return dict(dgh=_nan(g3), dgh_lp=_nan(g3, T) if lp else None, dgi=_nan(g3),
                dgi_lp=_nan(g3, T) if xcd else None, bsum=_nan((B, 4 * D)) if xcd else None,
                ddir0=_nan((B, D)))


def _cpu(*dicts):
    """The written tensors of the buffer dicts, on the host, NaN-free."""
    res = {}
    for d in dicts:
        for k, v in d.items():
            if v is not None:
                res[k] = v.cpu()
                assert not torch.isnan(res[k].float()).any(), k + ' has unwritten elements'
    return res


def _layer(hip, T, B, D, Fr, x, want):
    """Forward and backward through the layer entries; the plan must say `want`."""
    be, nf, nb = hip.gru_layer_plan(T, B, D)
    assert be == want
    p, dc = hip.ptr, hip.dcode(T)
    f = _fwd_bufs(T, B, D, Fr, be == 'xcd')
    wf, wb = _work(nf), _work(nb)
    hip.lib().call('srnn_gru_layer_fwd', dc, B, D, Fr, p(x['gi']), Fr * 3 * D, 3 * D, p(x['h0']),
                   p(x['whh']), p(x['bhh']), p(f['out']), p(f['out_lp']), Fr * D, D,
                   p(f['gates']), Fr * 4 * D, 4 * D, p(f['hprev']), p(wf) if nf else None, nf,
                   hip.stream())
    b = _bwd_bufs(T, B, D, Fr, be == 'xcd')
    hip.lib().call('srnn_gru_layer_bwd', dc, B, D, Fr, p(x['dy']), Fr * D, D, p(f['gates']),
                   Fr * 4 * D, 4 * D, p(f['out']), Fr * D, D, p(x['h0']), p(x['whh']),
                   p(x['whh_t']), p(b['dgh']), p(b['dgh_lp']), p(b['dgi']), p(b['dgi_lp']),
                   p(b['bsum']), Fr * 3 * D, 3 * D, p(b['ddir0']), p(wb) if nb else None, nb,
                   hip.stream())
    torch.cuda.synchronize()
    if be == 'xcd':     # the back end's own area comes first: word 0 is its error word
        assert hip.lib().dll.srnn_gru_xcd_error(p(wf)) == 0
        assert hip.lib().dll.srnn_gru_xcd_error(p(wb)) == 0
    assert hip.lib().dll.srnn_persistent_error_take() == 0
    return _cpu(f, b)


def _forced_xcd(hip, B, D, Fr, x):
    p = hip.ptr
    nf, nb = hip.gru_xcd_work_bytes(BF, B, D), hip.gru_xcd_bwd_work_bytes(BF, B, D)
    assert nf and nb
    f, b = _fwd_bufs(BF, B, D, Fr, True), _bwd_bufs(BF, B, D, Fr, True)
    wf, wb = _work(nf), _work(nb)
    hip.lib().call('srnn_gru_xcd_fwd2', hip.BF16, B, D, Fr, p(x['gi']), Fr * 3 * D, 3 * D,
                   p(x['h0']), p(x['whh']), p(x['bhh']), p(f['out']), p(f['out_lp']), Fr * D, D,
                   p(f['gates']), Fr * 4 * D, 4 * D, p(f['hprev']), p(wf), nf, hip.stream())
    hip.lib().call('srnn_gru_xcd_bwd2', hip.BF16, B, D, Fr, p(x['dy']), Fr * D, D, p(f['gates']),
                   Fr * 4 * D, 4 * D, p(f['out']), Fr * D, D, p(x['h0']), p(x['whh_t']),
                   p(b['dgh']), p(b['dgh_lp']), p(b['dgi']), p(b['dgi_lp']), p(b['bsum']),
                   Fr * 3 * D, 3 * D, p(b['ddir0']), p(wb), nb, hip.stream())
    torch.cuda.synchronize()
    assert hip.lib().dll.srnn_gru_xcd_error(p(wf)) == 0
    assert hip.lib().dll.srnn_gru_xcd_error(p(wb)) == 0
    return _cpu(f, b)


def _forced_seq(hip, B, D, Fr, x):
    p = hip.ptr
    assert hip.gru_seq_supported(BF, B, D)
    f, b = _fwd_bufs(BF, B, D, Fr, False), _bwd_bufs(BF, B, D, Fr, False)
    nw = (64 * ((B + 31) // 32) + 1) * 4
    wf, wb = _work(nw), _work(nw)
    h0T = x['h0'].to(BF)
    hip.lib().call('srnn_gru_seq_fwd', hip.BF16, B, D, Fr, p(x['gi']), Fr * 3 * D, 3 * D,
                   p(x['h0']), p(h0T), p(x['whh']), p(x['bhh']), p(f['out']), p(f['out_lp']),
                   Fr * D, D, p(f['gates']), Fr * 4 * D, 4 * D, p(wf), nw, hip.stream())
    hip.lib().call('srnn_gru_seq_bwd', hip.BF16, B, D, Fr, p(x['dy']), Fr * D, D, p(f['gates']),
                   Fr * 4 * D, 4 * D, p(f['out']), Fr * D, D, p(x['h0']), p(x['whh_t']),
                   p(b['dgh']), p(b['dgh_lp']), p(b['dgi']), Fr * 3 * D, 3 * D, p(b['ddir0']),
                   p(wb), nw, hip.stream())
    torch.cuda.synchronize()
    assert hip.lib().dll.srnn_persistent_error_take() == 0
    return _cpu(f, b)


def _step_loop(hip, T, B, D, Fr, x):
    """The per-step loops as the model ran them before the driver (and as
    test_gru_seq_*_matches_steps write them)."""
    p, dc = hip.ptr, hip.dcode(T)
    lp = T != torch.float32
    f, b = _fwd_bufs(T, B, D, Fr, False), _bwd_bufs(T, B, D, Fr, False)
    out, outT, gt = f['out'], f['out_lp'] if lp else f['out'], f['gates']
    h0T = x['h0'].to(T)
    gi = x['gi'].reshape(B * Fr, 3 * D)
    for t in range(Fr):
        hp_t, hp_f, ldh = (h0T, x['h0'], D) if t == 0 else (outT[:, t - 1], out[:, t - 1], Fr * D)
        hip.lib().call('srnn_gru_cell', dc, B, D, D, None, 0, None, None, p(gi[t:]), Fr * 3 * D,
                       p(hp_t), ldh, p(hp_f), ldh, p(x['whh']), p(x['bhh']), p(out[:, t]), Fr * D,
                       p(outT[:, t]) if lp else None, Fr * D, p(gt[:, t]), Fr * 4 * D,
                       hip.stream())
    dgh, dgi = b['dgh'], b['dgi']
    dghT = b['dgh_lp'] if lp else dgh
    ddir = [b['ddir0'], _nan((B, D))]
    for t in reversed(range(Fr)):
        nxt = t + 1 < Fr
        hp, ldhp = (out[:, t - 1], Fr * D) if t > 0 else (x['h0'], D)
        hip.lib().call('srnn_gru_cell_bwd', dc, B, D, p(x['dy'][:, t]), Fr * D,
                       p(dghT[:, t + 1]) if nxt else None, Fr * 3 * D,
                       p(ddir[(t + 1) % 2]) if nxt else None, p(x['whh']), p(x['whh_t']),
                       p(gt[:, t]), Fr * 4 * D, p(hp), ldhp, p(dgh[:, t]), Fr * 3 * D,
                       p(dghT[:, t]) if lp else None, Fr * 3 * D, p(dgi[:, t]), Fr * 3 * D,
                       p(ddir[t % 2]), hip.stream())
    torch.cuda.synchronize()
    return _cpu(f, b)


def _same(got, ref):
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


@pytest.fixture
def switches(monkeypatch):
    """Sets the two plan switches: switches('xcd' | 'seq' | 'steps') leaves that plan first."""
    def put(plan):
        for name, off in (('SRNN_GRU_XCD', ('seq', 'steps')), ('SRNN_GRU_SEQ', ('steps',))):
            if plan in off:
                monkeypatch.setenv(name, '0')
            else:
                monkeypatch.delenv(name, raising=False)
    put('xcd')
    return put


def test_layer_xcd_matches_forced(hip, switches):
    B, D, Fr = 20, 256, 3           # a row tail inside a 16-row tile
    x = _inputs(BF, B, D, Fr)
    _same(_layer(hip, BF, B, D, Fr, x, 'xcd'), _forced_xcd(hip, B, D, Fr, x))


def test_layer_seq_matches_forced(hip, switches):
    B, D, Fr = 40, 128, 3           # crosses the 32-row tile; D % 256 != 0, so XCD declines
    x = _inputs(BF, B, D, Fr)
    _same(_layer(hip, BF, B, D, Fr, x, 'seq'), _forced_seq(hip, B, D, Fr, x))


def test_layer_steps_bf16_matches_loop(hip, switches):
    B, D, Fr = 5, 256, 3
    x = _inputs(BF, B, D, Fr)
    switches('steps')
    _same(_layer(hip, BF, B, D, Fr, x, 'steps'), _step_loop(hip, BF, B, D, Fr, x))


@pytest.mark.parametrize('B,D,Fr', [(5, 48, 3), (5, 256, 3)])      # plain / deep-ring cells
def test_layer_steps_fp32_matches_loop(hip, switches, B, D, Fr):
    T = torch.float32
    x = _inputs(T, B, D, Fr)
    _same(_layer(hip, T, B, D, Fr, x, 'steps'), _step_loop(hip, T, B, D, Fr, x))


def test_layer_xcd_row_chunks(hip, switches):
    """A device shared 8 ways holds 64 rows of D = 1024 per launch (on 256 CUs): 80 rows run
    as launches of 64 + 16 rows over GruLayerFwd / GruLayerBwd::rows(), and give what the one
    launch of the unshared device gives."""
    B, D, Fr = 80, 1024, 3
    x = _inputs(BF, B, D, Fr)
    whole = _layer(hip, BF, B, D, Fr, x, 'xcd')
    share = hip.lib().dll.srnn_device_share()
    try:
        hip.set_device_share(8)
        chunked = _layer(hip, BF, B, D, Fr, x, 'xcd')
    finally:
        hip.set_device_share(share)
    _same(chunked, whole)


# ---- end to end: one conditioned tier's forward + backward under each plan
def tier_hashes(plan_name):
    """SHA-256 of every output and gradient of one tier_forward + tier_backward ([16, 4]
    frames, D = 256, B = 16, conditioned, bf16), and the model's GRU counters.  The caller has
    set the switches for `plan_name`; a job script runs this on two trees to compare them."""
    import model as M
    import samplernn_hip as H
    B, D, Fr, nfs, fs, C, S = 16, 256, 4, 16, 4, 20, 6
    torch.manual_seed(11)
    tier = M.FrameLevelRNN(fs, nfs, 1, D, True, True, C, S, True, False).to(DEV)
    tier.T = BF
    g = torch.Generator().manual_seed(12)
    prev = torch.randn(B, Fr, nfs, generator=g).to(DEV)
    cond = torch.randn(B, Fr, C, generator=g).to(DEV)
    spk = torch.randint(0, S, (B, 1), generator=g).to(DEV)
    dY = (torch.randn(B, Fr * fs, D, generator=g) * 0.1).to(DEV)
    before = dict(M._STATS)
    with torch.no_grad():
        ps = [q.detach() for q in tier._param_list()]
        Y, h_new, ctx = M.tier_forward(tier, prev, None, cond, spk, None, tier.h0.detach(), ps)
        _, dh0, grads = M.tier_backward(ctx, dY, True)
    torch.cuda.synchronize()
    assert H.lib().dll.srnn_persistent_error_take() == 0
    named = [('Y', Y), ('h_new', h_new), ('dh0', dh0)] + \
        [('grad%02d' % i, t) for i, t in enumerate(grads)]
    hashes = {}
    for k, t in named:
        t = t.detach().contiguous().cpu()
        assert torch.isfinite(t.float()).all(), k
        hashes[k] = hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()
    stats = {k: M._STATS[k] - before[k] for k in
             ('gru_xcd_fwd', 'gru_seq', 'gru_cell_steps', 'gru_xcd_bwd', 'gru_cell_bwd_steps')}
    return hashes, stats, Fr


@pytest.fixture(scope='module')
def tier_runs():
    return {}


@pytest.mark.parametrize('plan_name', ['xcd', 'seq', 'steps'])
def test_tier_end_to_end(hip, switches, tier_runs, plan_name):
    """Each plan runs the tier and bumps its own counters; gru_seq and the steps, which share
    their arithmetic, give the same bits in every output and gradient."""
    switches(plan_name)
    hashes, stats, Fr = tier_hashes(plan_name)
    print(plan_name, stats, hashes)
    assert stats == {'gru_xcd_fwd': int(plan_name == 'xcd'), 'gru_seq': int(plan_name == 'seq'),
                     'gru_cell_steps': Fr if plan_name == 'steps' else 0,
                     'gru_xcd_bwd': int(plan_name == 'xcd'),
                     'gru_cell_bwd_steps': Fr if plan_name == 'steps' else 0}
    tier_runs[plan_name] = hashes
    if plan_name == 'steps' and 'seq' in tier_runs:
        assert hashes == tier_runs['seq']
