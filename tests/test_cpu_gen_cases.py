"""The generation conformance sweep proven without a device (tests/gen_cases.py).

* every method A case is exact by itself: the float64 reference gives the same stream, logits
  and state with the bf16 rounding points on and off, in both summation orders of every matmul
  and in every association the model admits; every gate argument is saturated with margin, every
  draw margin is >= 1e-4, every stored value is representable;
* every influence the issue lists decides a gate somewhere in every model;
* the tables reach what they claim: models, widths, batches, n_cond, every kernel form x dtype x
  control level, both sides of every condition of the plan, fold_ok, fold_top and the tier-input
  LDS split;
* each built-in defect of the reference is reported by the checkers, by element, in a GPU-table
  case.
"""
import numpy as np
import pytest

import gen_cases as G

TABLE_A = G.table_a()


def _unique_inputs():
    seen, out = set(), []
    for c in TABLE_A + G.CARRY:
        k = (G._key(c.cfg), c.B, c.n_cond, c.forced)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def _same(a, b):
    if not (np.array_equal(a.seq, b.seq) and np.array_equal(a.logits, b.logits) and
            np.array_equal(a.state['hist'], b.state['hist'])):
        return False
    for x, y in zip(a.state['h'], b.state['h']):
        for p, q in zip(x, y):
            if not np.array_equal(p, q):
                return False
    for n in ('gh0', 'gh1'):
        if a.state[n] is not None and not np.array_equal(a.state[n], b.state[n]):
            return False
    return True


@pytest.mark.parametrize('c', _unique_inputs(), ids=lambda c: c.id)
def test_case_is_exact(c):
    model, cond, spk, noise, prefix, n_forced, ref = G.inputs(c)
    T = ref.logits.shape[1]
    kw = dict(prefix=prefix, n_forced=n_forced)
    mask = G.forced_margin_mask(c.B, T, n_forced)
    assert ref.margin[mask].min() >= G.MARGIN_MIN
    assert G.gate_margin(ref) >= G.GATE_MIN
    # the wide models cost seconds per run: there every association runs plain in order 0 (the
    # unfolded one is the run above) and rounded in the other order; the full crossing is made at
    # D <= 128
    combos = [(a, h, o) for a in G.ASSOCS if G.admits(c.cfg, a)
              for h in (G.hooks_off, G.hooks_bf16) for o in (0, 1)]
    if c.D > 128:
        combos = [x for x in combos if (x[1] is G.hooks_bf16 and x[2] == 1) or
                  (x[1] is G.hooks_off and x[2] == 0 and x[0] != 'unfolded')]
    for assoc, hooks, order in combos:
        r = G.reference(model, cond, spk, noise, assoc=assoc, hooks=hooks, order=order, **kw)
        assert G.gate_margin(r) >= G.GATE_MIN, (assoc, hooks.__name__, order)
        assert _same(r, ref), (assoc, hooks.__name__, order)
    # what is stored in bf16, and what is compared bit for bit in fp32, is representable
    seen, r = G.stored_values(model, cond, spk, noise, **kw)
    for name, x in seen:
        assert G.bf16_exact(x), name
    for x in [v for hk in r.state['h'] for v in hk] + [r.logits] + \
            [v for v in (r.state['gh0'], r.state['gh1']) if v is not None]:
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
        assert np.abs(x).max() < 2 ** 20 and np.array_equal(x * 2, np.round(x * 2))
    # a zero n exists in the table's models only through exact zeros
    assert all(np.array_equal(an == 0, zn & (an == 0)) for *_, an, zn in r.gates)


def _by_model():
    keys = {}
    for c in TABLE_A + G.CARRY:
        keys.setdefault(G._key(c.cfg), []).append(c)
    return keys


def _shortest(cs):
    """The cheapest free-running case of a model with more than one row."""
    return min((c for c in cs if c.forced is None and c.B > 1), key=lambda c: c.B * c.n_cond)


@pytest.mark.parametrize('c', [_shortest(cs) for cs in _by_model().values()], ids=lambda c: c.id)
def test_every_influence_decides_a_gate(c):
    """In every model of the table (each width draws its own weights), in its shortest case."""
    fs = c.fs
    model, cond, spk, noise, _, _, ref = G.inputs(c)
    cuts = ['samples', 'cond', 'spk', 'whh'] + (['upper'] if len(fs) > 1 else [])
    for cut in cuts:
        r = G.reference(model, cond, spk, noise, cut=cut)
        assert not _same(r, ref), cut
    # units whose n is exactly 0 occur (b_hh's n block inside the r product shows only there)
    assert any((zn & (an == 0)).any() for *_, an, zn in ref.gates)


def test_mlp_operands_over_the_table():
    """What the MLP part of the design relies on, over the table's own runs.  Logits are integers
    of moderate spread (per-step standard deviation 4 .. 16, the "about +-8" of the draw staying
    random) and far below 2^24.  W_hid and W_out are dense, so element [e, d] meets a non-zero
    operand exactly when unit d of a1 (a2 for W_out) is non-zero somewhere: at every width the
    [16, 2] model's runs activate >= 95 % of a1 and every unit of a2.  A unit of a1 needs one of
    its 6 Q / D levels at its tap, so the short runs of the other wide models reach fewer
    ([4, 2] at D = 1024, 8 steps: a quarter); the W_hid columns of the units they miss are
    compared through the [16, 2] model of that width only."""
    for key, cs in _by_model().items():
        fs, D = key[0], key[1]
        a1, a2 = np.zeros(D, dtype=bool), np.zeros(D, dtype=bool)
        for c in cs:
            ref = G.inputs(c)[-1]
            a1 |= ref.act1
            a2 |= ref.act2
            assert 4.0 <= ref.logits.std(-1).mean() <= 16.0, c.id
            assert np.abs(ref.logits).max() < 2 ** 12 and \
                np.array_equal(ref.logits, np.round(ref.logits)), c.id
        model = G.int_model(cs[0].cfg)[1]
        for name in ('hidden', 'output'):
            w = model['model.sample_level_mlp.%s.weight' % name]
            assert 0.6 < (w != 0).mean() < 0.72 and np.abs(w).max() == 1, (key, name)
        if fs == (16, 2):
            assert a1.mean() >= 0.95 and a2.all(), (key, a1.mean(), a2.mean())


def test_reference_carries_state():
    for c in G.CARRY[:6]:
        model, cond, spk, noise, _, _, ref = G.inputs(c)
        L = int(np.prod(c.fs))
        rs, f0, seqs, lps = None, 0, [], []
        for n in G.SPLITS:
            rs = G.reference(model, cond[:, f0:f0 + n], spk, noise[f0 * L:(f0 + n) * L],
                             state=rs.state if rs else None)
            seqs.append(rs.seq[:, L:])
            lps.append(rs.logits)
            # the part cut out of the one run is the chained call, state included
            p = G.part(ref, c.cfg, f0, n)
            assert np.array_equal(p.logp, rs.logp) and _same(p, rs)
            assert p.state['steps'] == rs.state['steps']
            f0 += n
        assert np.array_equal(np.concatenate(seqs, 1), ref.seq[:, L:])
        assert np.array_equal(np.concatenate(lps, 1), ref.logits)
        rs.seq = ref.seq
        rs.logits = ref.logits
        assert _same(rs, ref) and rs.state['steps'] == ref.state['steps']


def test_table_coverage():
    t = TABLE_A
    assert 150 <= len(t) + 2 * len(G.CARRY) + len(G.TABLE_T) <= 250
    have = lambda **kw: [c for c in t                                     # noqa: E731
                         if all(getattr(c, k) == v for k, v in kw.items())]
    for fs, kw in G.MODELS:
        for dt in G.DT:
            assert have(fs=tuple(fs), dtype=dt, **kw), (fs, kw, dt)
    for D in (16, 48, 64, 128, 256, 512, 80, 1024):
        for dt in G.DT:
            assert have(D=D, dtype=dt), (D, dt)
    assert have(D=1024, fs=(16, 2)) and have(D=1024, fs=(4, 2))
    for B in (1, 8, 9, 17):
        assert have(B=B)
    for n in (1, 2, 3, 5, 7):
        assert have(n_cond=n)
    for n in (5, 7):
        assert have(n_cond=n, graph=True) and have(n_cond=n, graph=False)
    assert all(have(fs=(16, 3), n_cond=n) for n in (2, 3, 5))
    for sw in G.SWITCHES:
        assert have(env={sw: '0'}, D=64) and have(env={sw: '0'}, D=1024)
    assert have(persistent=False, D=64) and have(persistent=False, D=1024)
    # every kernel form, dtype and control level meet
    forms = {}
    for c in t:
        r = G.route(c.cfg, c.dtype, c.B, c.env, c.persistent)
        if r.loop:
            forms.setdefault((r.form, c.dtype), set()).add(c.level)
    names = {f for f, _ in forms}
    for want in ('<1,4,16,MAXT=15>', '<1,4,16,FS0C=16>', '<1,4,16,MAXT=31>', '<2,4,4,MAXT=15>',
                 '<2,4,4,FS0C=16>', '<2,4,4,MAXT=31>', '<4,4,2,MAXT=15>', '<4,4,2,FS0C=16>',
                 '<4,4,2,MAXT=31>', 'bf16<4,4,2,1024>', 'fp32<8,4,1,1024>'):
        assert want in names, want
    for (form, dt), levels in forms.items():
        assert levels == {0, 1, 2}, (form, dt, levels)
    # the folded bf16 ticks (dim % 128 == 0) run through eager block, captured block, replays
    # and odd block, with fold_top and with the D = 1024 in-launch tick GEMM
    for D in (128, 1024):
        for n in (5, 7):
            for g in (True, False):
                cs = have(dtype='bf16', D=D, n_cond=n, graph=g, env={})
                assert any(G.route(c.cfg, 'bf16', c.B).fold_top for c in cs), (D, n, g)
    # both sides of the plan's conditions
    assert G.mlp_form('fp32', 9, 80, 16) is None and G.mlp_form('bf16', 9, 80, 4) is None
    assert G.mlp_form('fp32', 9, 1024, 4) is None and G.mlp_form('bf16', 9, 1024, 4)
    assert G.mlp_form('bf16', 9, 64, 32) and G.mlp_form('bf16', 9, 64, 33) is None
    routes = [(c, G.route(c.cfg, c.dtype, c.B, c.env, c.persistent)) for c in t]
    assert any(r.form is None for _, r in routes) and any(not r.loop and r.form for _, r in routes)
    # fold_ok: each conjunct false alone somewhere, and true
    fold = lambda **kw: [r.fold for c, r in routes                       # noqa: E731
                         if all(getattr(c, k) == v for k, v in kw.items())]
    assert any(fold(dtype='bf16')) and any(fold(dtype='fp32'))
    assert not any(fold(dtype='fp32', D=48)) and any(fold(dtype='fp32', D=64))      # dim % 64
    assert not any(fold(dtype='bf16', D=64)) and any(fold(dtype='bf16', D=128))     # dim % 128
    assert not any(fold(fs=(4,))) and not any(fold(n_rnn=2))
    assert not any(fold(fs=(20, 2))) and not any(fold(fs=(32, 2)))                   # nfs <= 16
    assert not any(fold(fs=(2, 9)))                                                  # FS1 <= 8
    assert not any(fold(env={'SRNN_GEN_FOLD': '0'}))
    assert not any(fold(env={'SRNN_GEN_FOLD_F32': '0'}, dtype='fp32'))
    assert all(fold(env={'SRNN_GEN_FOLD_F32': '0'}, dtype='bf16', D=128))
    # fold_top: two tiers, in_dim <= TA_AP, the switch
    ftop = lambda **kw: [r.fold_top for c, r in routes                   # noqa: E731
                         if r.fold and all(getattr(c, k) == v for k, v in kw.items())]
    assert all(ftop(fs=(16, 2), cond_dim=6, env={})) and not any(ftop(fs=(4, 2, 2)))
    assert not any(ftop(cond_dim=86)) and not any(ftop(env={'SRNN_GEN_FOLD_TOP': '0'}))
    assert 16 * 4 + 86 > G.TA_AP
    # the tier-input LDS split
    paths = {p for _, r in routes for p in r.inputs}
    assert paths == {'tiled', 'raised', 'row'}
    assert G.tier_input_path(227) == 'tiled' and G.tier_input_path(228) == 'raised'
    assert G.tier_input_path(567) == 'raised' and G.tier_input_path(569) == 'row'
    # forced lengths 0, 1, FS0 - 1, FS0, FS0 + 1, L, T all occur
    c = have(forced='mixed', fs=(16, 2), D=64)[0]
    assert set(G.forced_lengths(c).tolist()) == {0, 1, 15, 16, 17, 32, 64}
    # method T: the cases of the issue, each on its paths
    tt = {(c.fs, c.D, c.dtype, c.n_rnn) for c in G.TABLE_T}
    for want in [((16, 4), D, dt, 1) for D in (64, 128, 1024) for dt in G.DT] + \
            [((4, 2, 2), 64, dt, 1) for dt in G.DT] + [((20, 4), 32, dt, 2) for dt in G.DT]:
        assert want in tt, want
    assert {c.assoc for c in G.TABLE_T} == set(G.ASSOCS)


# defect -> a GPU-table case that shows it, and what the report must name
DEFECT_CASES = {
    'taps_reversed': G.case((16, 2), 64, 'bf16', 9, 3),
    'fi_off_by_one': G.case((4, 2, 2), 128, 'bf16', 9, 3),
    'cond_frame': G.case((16, 2), 64, 'fp32', 9, 3),
    'noise_bt': G.case((16, 2), 64, 'fp32', 9, 3),
    'upsample_order': G.case((16, 2), 64, 'bf16', 9, 3),
    'bhh_n_outside': G.case((16, 2), 64, 'bf16', 9, 3),
    'stale_h_group': G.case((16, 2), 64, 'bf16', 17, 2),
    'ragged_last_row': G.case((16, 2), 64, 'bf16', 12, 2),
    'spk_other_row': G.case((4, 2), 64, 'bf16', 9, 3),
    'kunit_twice': G.case((16, 2), 48, 'bf16', 9, 2),
    'tick_parity': G.case((16, 3), 64, 'bf16', 9, 3),
    'forced_no_noise': G.case((16, 2), 64, 'bf16', 9, 2, forced='mixed'),
}


@pytest.mark.parametrize('defect', G.DEFECTS)
def test_defect_is_reported(defect):
    c = DEFECT_CASES[defect]
    assert c.id in {x.id for x in TABLE_A}, 'the defect must show in a case the GPU runs'
    model, cond, spk, noise, prefix, n_forced, ref = G.inputs(c)
    r = G.route(c.cfg, c.dtype, c.B, c.env, c.persistent)
    bits = (1 if r.fold else 0) | (2 if r.fold_top else 0)
    # the clean reference dressed as a device result passes
    seq, lp, rec = G.reference_as_result(ref, c.cfg, r.fold)
    rec['hdr'][:] = np.array([0x314E5253, c.dtype == 'bf16', len(c.fs), c.n_rnn, c.D,
                              int(np.prod(c.fs)), bits, 0], dtype=np.uint32)
    assert G.check_case(seq, lp, rec, ref, c.cfg, c.dtype, bits, G.C_LSE) == []
    bad = G.reference(model, cond, spk, noise, prefix=prefix, n_forced=n_forced, defect=defect)
    bseq, blp, brec = G.reference_as_result(bad, c.cfg, r.fold)
    brec['hdr'][:] = rec['hdr']
    msgs = G.check_case(bseq, blp, brec, ref, c.cfg, c.dtype, bits, G.C_LSE)
    assert msgs, defect
    text = ' | '.join(msgs)
    # the first element named is the first that differs
    if not np.array_equal(bad.seq, ref.seq):
        b, col = np.argwhere(bad.seq != ref.seq)[0]
        assert 'seq[row %d, column %d]' % (b, col) in text, text
        rows = set(np.argwhere(bad.seq != ref.seq)[:, 0].tolist())
    else:
        # only the returned state differs (tick_parity)
        assert 'h[tier' in text and 'unit' in text, text
        rows = set(range(c.B))
    if defect == 'stale_h_group':
        assert rows <= set(range(8, 16)), rows
    if defect == 'ragged_last_row':
        assert rows <= set(range((c.B // 8) * 8, c.B - 1)), rows
    if defect == 'forced_no_noise':
        assert rows <= set(np.nonzero(n_forced > 0)[0].tolist()), rows
        b, col = np.argwhere(bad.seq != ref.seq)[0]
        assert col - int(np.prod(c.fs)) >= n_forced[b]
    if defect == 'tick_parity':
        assert np.array_equal(bad.seq, ref.seq)


def test_method_t_bounds_small():
    """The bounds of method T come from the references alone: the oracle's fp32 rounding (E32)
    and the reference's own bf16 rounding points (E16), both far below today's 0.25 / 0.02."""
    for c in G.TABLE_T:
        if c.D > 128:
            continue
        *_, ref, b = G.inputs_t(c)
        assert np.isfinite(ref.logp).all() and 0 < b.e_lp and 0 < b.e_h
        if c.dtype == 'fp32':
            assert b.e_lp < 1e-4, (c.id, b.e_lp)
        else:
            assert 1e-4 < b.e_lp < 0.25 and b.e_mean < 0.02, (c.id, b.e_lp, b.e_mean)


def test_rounding_and_bound_helpers():
    assert G.bf16_round(np.array([1.00390625]))[0] == 1.0            # tie to even
    assert G.bf16_round(np.array([1.01171875]))[0] == 1.015625
    assert G.bf16_exact([256.0, 0.5, 2.0 ** 30, -44.0]) and not G.bf16_exact([257.0, 128.5])
    assert G.ulp32(np.array([1.0]))[0] == 2.0 ** -23 and G.ulp32(np.array([-5.0]))[0] == 2.0 ** -21
    lut = G.lut2()
    assert lut[128] == 0.0 and abs(abs(lut[127]) - 3.48e-4) < 1e-6 and abs(lut[0] + 2.0) < 1e-12
    with pytest.raises(AssertionError):
        G.check_logp(np.zeros((1, 1, 256)), type('R', (), {'logp': np.zeros((1, 1, 256))}), 65)
