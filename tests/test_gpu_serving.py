"""Continuous batching on the device: per-row Philox origins (Generator stream_ids=;
srnn_generate6), fresh records (Generator.fresh_state; srnn_gen_state_fresh) and Generator.serve.

The contract: a stream is the same stream -- indices and log-probs, torch.equal -- whichever row
of a call serves it and whatever the other rows of the call are doing, so every utterance served
from a slot is the utterance generated alone (at the same batch size).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipe
from test_gpu_streaming import BF16, DEV, F32, L, assert_same, build, inputs, run

pytestmark = pytest.mark.gpu
B = 5
LENGTHS = [3, 1, 2, 4, 1, 2, 1]


# ------------------------------------------------------------------ fresh records
@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('name', ['t3', 't4la', 't3r2wn', 't2'])
def test_fresh_equals_none(hip, name, dtype, persistent):
    import model as M
    m, cfg = build(name, dtype)
    cond, spk, _ = inputs(cfg, B, 2)
    fresh = M.Generator(m, True).fresh_state(B)
    assert fresh.steps.tolist() == [0] * B and fresh.n_seqs == B
    assert bool((fresh.blob == fresh.blob[0]).all()), 'fresh records differ between rows'
    kw = dict(sampler='philox', seed=41, persistent=persistent)
    none = run(m, B, cond, spk, **kw)
    got = run(m, B, cond, spk, state=fresh, **kw)
    assert_same(got, none)
    assert torch.equal(got[2].blob, none[2].blob)
    assert got[2].steps.tolist() == [2 * m.lookback] * B


# ------------------------------------------------------------------ per-row origins
@pytest.fixture(scope='module')
def refs():
    """Per (dtype, persistent, level): ref1 = 3 frames with Philox rows 10..14 and the state after
    its first 2; ref2 = 1 frame of another cond with rows 20..24.  level 0: no controls; 1:
    per-row temperature / top_k; 2: and top_p."""
    cache = {}

    def get(dtype, persistent, level=0):
        key = (dtype, persistent, level)
        if key not in cache:
            m, cfg = build('t3', dtype)
            cond1, spk, _ = inputs(cfg, B, 3, seed=8)
            cond2, _, _ = inputs(cfg, B, 1, seed=31)
            ctl = [{}, {}]
            if level >= 1:
                ctl[0] = dict(temperature=[1.0, 0.7, 0.0, 1.3, 0.9], top_k=[0, 40, 3, 256, 17])
                ctl[1] = dict(temperature=[0.8, 1.0, 1.1, 0.6, 1.0], top_k=[9, 0, 0, 30, 0])
            if level >= 2:
                ctl[0]['top_p'] = [1.0, 0.9, 0.5, 0.8, 0.95]
                ctl[1]['top_p'] = [0.7, 1.0, 0.9, 0.85, 1.0]
            kw = dict(sampler='philox', seed=1234, persistent=persistent)
            one = run(m, B, cond1, spk, row_offset=10, **kw, **ctl[0])
            head = run(m, B, cond1[:, :2], spk, row_offset=10, **kw, **ctl[0])
            two = run(m, B, cond2, spk, row_offset=20, **kw, **ctl[1])
            cache[key] = dict(m=m, cfg=cfg, cond1=cond1, cond2=cond2, spk=spk, kw=kw, one=one,
                              head=head, two=two, ctl=ctl)
        return cache[key]
    return get


@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_permuted_philox_continuation(hip, refs, dtype, persistent):
    r = refs(dtype, persistent)
    perm = [3, 0, 4, 2, 1]
    got = run(r['m'], B, r['cond1'][perm, 2:], r['spk'][perm], state=r['head'][2].rows(perm),
              stream_ids=[10 + p for p in perm], **r['kw'])
    assert torch.equal(got[0], r['one'][0][perm, 2 * L:])
    assert torch.equal(got[1], r['one'][1][perm, 2 * L:])
    assert torch.equal(got[2].blob, r['one'][2].blob[perm])
    # the ids are what moved the rows' noise: without them the permuted rows draw other samples
    wrong = run(r['m'], B, r['cond1'][perm, 2:], r['spk'][perm], state=r['head'][2].rows(perm),
                row_offset=10, **r['kw'])
    assert not torch.equal(wrong[0], got[0])


def _mixed(r, **kw):
    """Rows 0-2 continue ref1 after 2 frames, rows 3-4 start ref2's streams 23, 24."""
    import model as M
    gen = M.Generator(r['m'], True)
    state = gen.fresh_state(B).replace([0, 1, 2], r['head'][2].rows([0, 1, 2]))
    assert state.steps.tolist() == [2 * L] * 3 + [0, 0]
    cond = np.concatenate([r['cond1'][:3, 2:3], r['cond2'][3:, :1]])
    ctl = {k: list(r['ctl'][0][k][:3]) + list(r['ctl'][1][k][3:]) for k in r['ctl'][0]}
    return run(r['m'], B, cond, r['spk'], state=state, stream_ids=[10, 11, 12, 23, 24],
               **dict(r['kw'], **kw), **ctl)


def _check_mixed(r, got):
    assert torch.equal(got[0][:3], r['one'][0][:3, 2 * L:]), 'continued rows: indices'
    assert torch.equal(got[1][:3], r['one'][1][:3, 2 * L:]), 'continued rows: log-probs'
    assert torch.equal(got[0][3:], r['two'][0][3:, :L]), 'fresh rows: indices'
    assert torch.equal(got[1][3:], r['two'][1][3:, :L]), 'fresh rows: log-probs'
    assert got[2].steps.tolist() == [3 * L] * 3 + [L] * 2
    assert torch.equal(got[2].blob[:3], r['one'][2].blob[:3])
    assert torch.equal(got[2].blob[3:], r['two'][2].blob[3:])


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_mixed_step_counts(hip, refs, dtype, persistent, use_graph):
    r = refs(dtype, persistent)
    if persistent:
        assert hip.gen_persistent_rows(dtype, B, r['cfg']['dim'], 16) > 0
    _check_mixed(r, _mixed(r, use_graph=use_graph))


def test_mixed_step_counts_noise_in_loop(hip, refs, monkeypatch):
    """SRNN_GEN_NOISE_AHEAD=0: a call with per-row origins still draws ahead (no build of the
    persistent loop's own draw knows them)."""
    r = refs(BF16, True)
    monkeypatch.setenv('SRNN_GEN_NOISE_AHEAD', '0')
    _check_mixed(r, _mixed(r))


@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('level', [1, 2])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_mixed_step_counts_with_controls(hip, refs, dtype, level, persistent):
    """Per-row temperature / top_k (level 1) and top_p (level 2), and row 1 forced along the first
    20 samples of its own continuation: the controlled builds under per-row origins."""
    r = refs(dtype, persistent, level)
    if persistent:
        assert hip.gen_persistent_rows(dtype, B, r['cfg']['dim'], 16, ctrl=level) > 0
    _check_mixed(r, _mixed(r))
    prefix = torch.full((B, 20), 128, dtype=torch.long)
    prefix[1] = r['one'][0][1, 2 * L:2 * L + 20]
    _check_mixed(r, _mixed(r, prefix=prefix, prefix_len=[0, 20, 0, 0, 0]))


def test_mixed_step_counts_per_sample_plan(hip):
    """dim 80 has no persistent plan (gen_persistent_rows == 0): the per-sample sampler kernel is
    taken by plan, not by flag, and applies the rows' origins itself."""
    import model as M
    cfg = dict(recipe.CONFIGS['t3'], dim=80)
    assert hip.gen_persistent_rows(F32, B, 80, 16) == 0
    m = M.SampleRNN(cfg['frame_sizes'], cfg['n_rnn'], cfg['dim'], cfg['learn_h0'],
                    cfg['q_levels'], True, cfg['weight_norm'], cfg['cond_dim'], cfg['spk_dim'])
    M.Predictor(m).load_state_dict({k: torch.from_numpy(v.copy())
                                    for k, v in recipe.make_weights(cfg, 7).items()})
    m = m.to(DEV)
    cond1, spk, _ = inputs(cfg, B, 3, seed=8)
    cond2, _, _ = inputs(cfg, B, 1, seed=31)
    kw = dict(sampler='philox', seed=5)
    r = dict(m=m, cfg=cfg, cond1=cond1, cond2=cond2, spk=spk, kw=kw, ctl=[{}, {}],
             one=run(m, B, cond1, spk, row_offset=10, **kw),
             head=run(m, B, cond1[:, :2], spk, row_offset=10, **kw),
             two=run(m, B, cond2, spk, row_offset=20, **kw))
    _check_mixed(r, _mixed(r))


# ------------------------------------------------------------------ serve
def _requests(cfg, controls=False):
    reqs = []
    for u, n in enumerate(LENGTHS):
        rq = dict(cond=recipe.synth_cond((n, cfg['cond_dim']), 50 + u), spk=u % cfg['spk_dim'],
                  stream_id=100 + 3 * u)
        if controls and u % 2:
            rq.update(temperature=0.6 + 0.1 * u, top_k=[0, 30][u % 4 == 1])
        if controls and u in (2, 3):
            rq['top_p'] = 0.8
        reqs.append(rq)
    return reqs


@pytest.mark.parametrize('dtype,controls', [(F32, False), (BF16, False), (BF16, True)],
                         ids=['fp32', 'bf16', 'bf16-controls'])
def test_serve_equals_each_utterance_alone(hip, dtype, controls):
    import model as M
    m, cfg = build('t3', dtype)
    slots = 3
    for level in (0, 2) if controls else (0,):
        assert hip.gen_persistent_rows(dtype, slots, cfg['dim'], 16, ctrl=level) > 0
    reqs = _requests(cfg, controls)
    gen = M.Generator(m, True)
    got = list(gen.serve(reqs, slots, 2, seed=77))
    assert [u for u, _ in got] == [1, 2, 0, 4, 5, 3, 6]
    plan = M.serve_plan(LENGTHS, slots, 2)
    assert gen.last_serve == dict(calls=len(plan), frames=[n for n, _ in plan],
                                  row_frames=sum(slots * n for n, _ in plan))
    assert gen.last_serve['row_frames'] == 18
    for u, samples in got:
        rq = reqs[u]
        ctl = {k: rq[k] for k in ('temperature', 'top_k', 'top_p') if k in rq}
        want = gen(slots, 0, rq['cond'], rq['spk'], sampler='philox', seed=77,
                   row_offset=rq['stream_id'], **ctl)[0]
        assert samples.dtype == torch.float32 and not samples.is_cuda
        assert samples.shape == (LENGTHS[u] * L,)
        assert torch.equal(samples, want), 'request %d differs from the utterance alone' % u


# ------------------------------------------------------------------ entries, ops
def _op_args(m, cond, spk):
    import model as M
    weights, meta = M.generation_weights(m)
    condt = torch.from_numpy(cond).to(DEV, torch.float32).contiguous()
    row_bias = M.top_row_bias(m, torch.from_numpy(spk).to(DEV))
    return (weights, meta, condt, row_bias, None, 11, 3, 1, True)


def _raw(m, args, entry, rows=None, st=None):
    """One direct call of srnn_generate5 / 6 on a seq pre-filled like the op's; returns
    (return code, message, seq, logp)."""
    import model as M
    import samplernn_hip as H
    weights, meta, condt, row_bias = args[:4]
    sm = M.srnn_model_struct(weights, meta)
    n, T = condt.shape[0], condt.shape[1] * L
    seq = torch.full((n, L + T), 128, dtype=torch.long, device=DEV)
    logp = torch.zeros((T, n, 256), device=DEV)
    sz = ctypes.c_size_t(0)
    H.lib().call('srnn_gen_workspace_size', ctypes.byref(sm), n, ctypes.byref(sz))
    ws = torch.empty(sz.value, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    tail = [ctypes.byref(st) if st is not None else None]
    if entry == 'srnn_generate6':
        tail.append(ctypes.byref(rows) if rows is not None else None)
    rc = getattr(H.lib().dll, entry)(ctypes.byref(sm), n, condt.shape[1], H.ptr(condt),
                                     H.ptr(row_bias), None, 11, 3, H.ptr(seq), H.ptr(logp),
                                     H.ptr(ws), sz.value, 1, H.stream(), None, None, None, *tail)
    torch.cuda.synchronize()
    return rc, H.lib().dll.srnn_last_error().decode(), seq, logp


def test_entries_forward(hip):
    """srnn_generate5 is srnn_generate6 with rows = NULL, and both are the op with both arrays
    None; noise_row = row0 + b with step0 = 0 spelled out per row draws the same stream."""
    import samplernn_hip as H
    m, cfg = build('t3', F32)
    cond, spk, _ = inputs(cfg, B, 3)
    args = _op_args(m, cond, spk)
    none = (None, None, None, None, 0, None, None, False)
    want = torch.ops.srnn.generate_rows(*args, *none, None, None)
    base = torch.ops.srnn.generate_stream(*args, *none)
    assert torch.equal(want[0], base[0]) and torch.equal(want[1], base[1])
    for entry, rows in (('srnn_generate5', None), ('srnn_generate6', None),
                        ('srnn_generate6', H.SrnnGenRows())):
        rc, msg, seq, logp = _raw(m, args, entry, rows)
        assert rc == 0, msg
        assert torch.equal(seq, want[0]) and torch.equal(logp, want[1]), entry
    ids = torch.arange(3, 3 + B, dtype=torch.int32, device=DEV)
    zero = torch.zeros(B, dtype=torch.int64, device=DEV)
    spelled = torch.ops.srnn.generate_rows(*args, *none, ids, zero)
    assert torch.equal(spelled[0], want[0]) and torch.equal(spelled[1], want[1])


def test_row_origins_are_checked_before_anything_is_written(hip):
    import samplernn_hip as H
    m, cfg = build('t3', F32)
    cond, spk, _ = inputs(cfg, B, 1)
    args = _op_args(m, cond, spk)
    none = (None, None, None, None, 0, None, None, False)
    ok = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32, device=DEV)
    far = torch.tensor([0, 0, 0xFFFFFFFF - L + 1, 0, 0], dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match='32-bit'):
        torch.ops.srnn.generate_rows(*args, *none, ok, far)
    with pytest.raises(ValueError, match='noise_row'):
        torch.ops.srnn.generate_rows(*args, *none, ok - 1, None)
    with pytest.raises(ValueError, match='noise_row'):
        torch.ops.srnn.generate_rows(*args, *none, ok[:4], None)
    # the library's own checks (the op's never let these through)
    step32 = far.to(torch.int32)            # the low words: 0xFFFFFFC0 as uint32
    rows = H.SrnnGenRows(H.ptr(ok), H.ptr(step32))
    rc, msg, seq, logp = _raw(m, args, 'srnn_generate6', rows)
    assert rc == 1 and 'row 2: step0 4294967232 + 64 steps overflow' in msg, msg
    assert bool((seq == 128).all()) and bool((logp == 0).all())
    neg = ok - 1
    rc, msg, seq, _ = _raw(m, args, 'srnn_generate6', H.SrnnGenRows(H.ptr(neg), None))
    assert rc == 1 and 'noise_row[0] = -1 is negative' in msg, msg
    assert bool((seq == 128).all())
    # the last step that fits
    step32 = (far - (far > 0).long()).to(torch.int32)
    rc, msg, _, _ = _raw(m, args, 'srnn_generate6', H.SrnnGenRows(H.ptr(ok), H.ptr(step32)))
    assert rc == 0, msg


def test_opcheck_serving_ops(hip):
    m, cfg = build('t3', BF16)
    n = 3
    cond, spk, _ = inputs(cfg, n, 1)
    args = _op_args(m, cond, spk)
    st = torch.ops.srnn.gen_state_fresh(args[0], args[1], n)
    ids = torch.tensor([7, 7, 2], dtype=torch.int32, device=DEV)
    steps = torch.tensor([0, 64, 640], dtype=torch.int64, device=DEV)
    tau = torch.tensor([1.0, 0.7, 0.0], device=DEV)
    k = torch.tensor([0, 8, 0], dtype=torch.int32, device=DEV)
    utils = ('test_schema', 'test_faketensor')
    for extra in ((None, None, None, None, 0, None, None, True, None, None),
                  (None, None, None, st, 0, None, None, True, ids, steps),
                  (tau, k, None, st, 0, None, None, False, ids, None)):
        torch.library.opcheck(torch.ops.srnn.generate_rows.default, args + extra,
                              test_utils=utils)
    torch.library.opcheck(torch.ops.srnn.gen_state_fresh.default, (args[0], args[1], n),
                          test_utils=utils)


# ------------------------------------------------------------------ CLI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'jalil-saboorizadeh-multi-speaker-neural-vocoder_amd')


def test_cli_slots(hip, tmp_path):
    """generate.py --batch_files True --slots 2 --chunk_frames 2 writes what Generator.serve
    yields for the same files (9 and 7 frames, 2 samples each: stream ids j n + i), and refuses
    the host sampler."""
    import model as M
    from dataset import write_wav
    from test_cpu_data import _write_corpus
    cfg = dict(recipe.CONFIGS['t3_20_4'], spk_dim=2)            # lookback 80
    files = ['72e000', '75v000']
    _, cond = _write_corpus(str(tmp_path) + '/', files, frames=(9, 7))
    for s in ('72', '75'):
        os.symlink(tmp_path, os.path.join(cond, 'spk' + s))
    (tmp_path / 'generate_cond_gina.list').write_text('\n'.join(files) + '\n')
    (tmp_path / 'generate_spk_gina.list').write_text('72\n75\n')
    os.makedirs(tmp_path / 'npy_datasets')
    np.save(str(tmp_path / 'npy_datasets' / 'spk_id.npy'), np.array(['72', '75']))
    np.save(str(tmp_path / 'npy_datasets' / 'min_max_joint.npy'),
            np.stack([np.full(43, -1e4), np.full(43, 1e4)]))
    sd = {k: torch.from_numpy(v.copy()) for k, v in recipe.make_weights(cfg, 3).items()}
    exp = 'exp:S~frame_sizes:20,4~dim:32'
    os.makedirs(tmp_path / 'results' / exp / 'checkpoints')
    os.makedirs(tmp_path / 'results' / exp / 'samples')
    ck = 'results/%s/checkpoints/ep1-it1' % exp
    torch.save(sd, str(tmp_path / ck))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = [sys.executable, '-u', os.path.join(PKG, 'generate.py'), '--model', ck,
            '--datasets_path', str(tmp_path) + '/', '--cond_set', 'cond/', '--frame_sizes', '20',
            '4', '--n_rnn', '2', '--dim', '32', '--learn_h0', 'false', '--n_samples', '2',
            '--batch_files', 'true', '--slots', '2']
    r = subprocess.run(base + ['--sampler', 'torch'], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '--sampler philox' in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ['--sampler', 'philox', '--chunk_frames', '2'], cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # the same inputs through Generator.serve in this process
    import generate as G
    params = dict(G.default_params, frame_sizes=[20, 4], n_rnn=2, dim=32, learn_h0=False,
                  model=ck)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        m = G.build_model(params, 2, True)
        conds = [G.file_conditioning(str(tmp_path) + '/cond/' + f, j, params)
                 for j, f in enumerate(files)]
    finally:
        os.chdir(cwd)
    reqs = [dict(cond=conds[j], spk=j, stream_id=2 * j + i) for j in range(2) for i in range(2)]
    served = dict(M.Generator(m, True).serve(reqs, 2, 2, seed=G.default_params['seed']))
    for j, (f, s) in enumerate(zip(files, ('72', '75'))):
        name = tmp_path / 'results' / exp / 'samples' / ('ep1-it1_file-%s_spk-%s.wav' % (f, s))
        # (both samples of a file go to one name: the last one written stays)
        want = tmp_path / 'want.wav'
        write_wav(str(want), served[2 * j + 1].numpy(), sr=16000)
        assert name.read_bytes() == want.read_bytes()
        assert len(want.read_bytes()) > (9, 7)[j] * 80 * 2
