"""Cases, float64 reference and checkers of the generation conformance sweep.  Not a test module.

tests/test_gpu_gen_conformance.py runs the tables below on the device, tests/test_cpu_gen_cases.py
proves them without one.  `reference` calls neither the product nor the CPU oracle (only
oracle_run does, for method T's E32: the oracle's own deviation from `reference`): it is a
plain numpy float64 restatement of Generator.__call__ (every tier tick, the sample-level MLP, the
draw argmax(z - log q) with the first index on ties, the forced prefix, the carried state).

Method A -- the whole index stream bit for bit, from integer models (int_model):
  * everything that flows onward linearly is exact in fp32 and representable in bf16: h is in
    {0, +-1/2, +-1} (h0 in halves, afterwards a saturated GRU returns h or n in {-1, 0, 1}), the
    carried gh = W_hh h + b_hh are halves below 2^16, the upsampling rows, tab, a1, a2 and the
    logits are small integers or halves, cond is in quarters, the speaker path is integer;
  * gate arguments are not exact (the frame inputs 2 udequantize(x) are arbitrary fp32 values) but
    saturated: every r, z and non-zero n argument has magnitude >= GATE_MIN = 1024 under every
    association and with the bf16 rounding on or off, so sigmoid is exactly 0 / 1 and tanh exactly
    +-1 on the device (expf overflows above 88.73, tanhf saturates above 9.01).  n is exactly 0
    only through exact zeros (gi_n = 0 and r = 0): such units exist, they are where b_hh's n block
    inside the r product shows;
  * gate signs are decided by the frame's samples, the upper tier's row, the cond frame, the
    speaker row and h through W_hh, each somewhere in every model (test_cpu proves it);
  * W_hid and W_out are dense in small integers and a1 is sparse, its active set moving with the
    history; logits are integers of moderate spread, so the draw stays random;
  * the noise is replayed and seeded per case so that the smallest draw margin is >= 1e-4.

Method T -- teacher-forced random-weight models (recipe.make_weights), every step compared with
this reference: fp32 within 4 x the CPU fp32 oracle's own deviation from it, bf16 within 2 x the
deviation that the rounding points below cause in this reference.

Rounding points (`hooks(name, x)`: where the product rounds to the model dtype), from generate.hip,
gen_mlp.hip, gen_rows.hip and model.generation_weights:
  'w'      every weight matrix (W_in, W_ih, W_hh, W_up, E, the MLP's W_in / W_hid / W_out), and so
           wcat = [W_up; W_hh], which is those rows again; biases, h0 and row_bias stay fp32
  'a'      the tier input operand: 2 udequantize(x) LUT values and the cond frame
  'atop'   the folded top tick's input row (the same values, TA_AP columns)
  'x'      the unfolded tier input x = W_in a + b + add
  'h_lp'   the copy of h the next GEMM reads (fp32 h is kept beside it)
  'wfold'  W_ih0 W_up1[j], the folded upper tick's weights
  'min1'   W_ih1 W_in1, the folded top tick's weights (Min of the bottom tick stays fp32)
  'tab'    Tab[k][q] = W_in[:, :, k] E[q]
  'a1'     relu(sum_k Tab[k][x_k] + up0)
  'a2'     relu(W_hid a1 + b_hid)
G, bfold, P1, the carried gh, the upsampling rows, the logits and log-probs are fp32.
"""
import functools
import types

import numpy as np

import recipe

Q = 256
GATE_MIN = 1024.0
MARGIN_MIN = 1e-4
FOLD_MAX_FS1, TA_AP, HIST = 8, 128, 32
HOOK_NAMES = ('w', 'a', 'atop', 'x', 'h_lp', 'wfold', 'min1', 'tab', 'a1', 'a2')
ASSOCS = ('unfolded', 'folded', 'folded_top')
DEFECTS = ('taps_reversed', 'fi_off_by_one', 'cond_frame', 'noise_bt', 'upsample_order',
           'bhh_n_outside', 'stale_h_group', 'ragged_last_row', 'spk_other_row', 'kunit_twice',
           'tick_parity', 'forced_no_noise')


# ---------------------------------------------------------------------------- number formats
def bf16_round(x):
    """float64 -> the nearest bf16 (ties to even, through fp32 as the device does), as float64."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)).view(np.uint32)
    b = ((b.astype(np.uint64) + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def bf16_exact(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.array_equal(bf16_round(x), x))


def hooks_off(name, x):
    return x


def hooks_bf16(name, x):
    return bf16_round(x)


def hooks_weights_only(name, x):
    return bf16_round(x) if name in ('w', 'wfold', 'min1', 'tab') else x


def ulp32(x):
    """Spacing of fp32 at |x| (float64 array)."""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def lut2():
    """2 udequantize(k), k < 256 (utils.py: iulaw(imidrise(k))), float64; level 128 is exactly 0."""
    c = np.arange(Q, dtype=np.float64) * 2.0 / Q - 1.0
    return 2.0 * np.sign(c) * (np.exp(np.abs(c) * np.log(256.0)) - 1.0) / 255.0


# ---------------------------------------------------------------------------- models
def config(frame_sizes, dim, n_rnn=1, cond_dim=6, spk_dim=4):
    return dict(frame_sizes=list(frame_sizes), n_rnn=n_rnn, dim=dim, q_levels=Q,
                weight_norm=False, cond_dim=cond_dim, spk_dim=spk_dim, learn_h0=True)


def _key(cfg):
    return (tuple(cfg['frame_sizes']), cfg['dim'], cfg['n_rnn'], cfg['cond_dim'], cfg['spk_dim'])


SAMPLE, UPPER, COND, SPK = 0, 1, 2, 3
P_SAMPLE, P_INT = 24, 14           # W_ih = 2^p: 2^24 * 3.5e-4 and 2^14 / 4 are both >= 4096
B_GATE = 2048.0                    # |b_ih| of a gate that its input may leave at exactly 0
W_REC, B_REC = 2.0 ** 14, 2048.5   # a gate decided by h through W_hh, and its b_hh


@functools.lru_cache(maxsize=None)
def _int_model(key, seed):
    fs, D, n_rnn, C, S = key
    cfg = config(fs, D, n_rnn, C, S)
    rng = np.random.Generator(np.random.PCG64(seed * 7919 + D * 31 + sum(fs)))
    nfs = recipe.cumprod(fs)
    nt = len(fs)
    sd = {}
    # x-unit classes of each tier: what the unit's value is made of (one source per unit, so no
    # two sources can cancel to something small)
    cls = []
    for k in range(nt):
        top = k == nt - 1
        c = np.where(np.arange(D) % 2 == 0, SAMPLE, UPPER)
        if top:
            c = np.where(np.arange(D) % 2 == 0, SAMPLE, np.where(np.arange(D) % 4 == 1, COND, SPK))
        cls.append(c)
    for k in range(nt):
        p = 'model.frame_level_rnns.%d.' % k
        top = k == nt - 1
        n = nfs[k]
        sd[p + 'h0'] = rng.integers(-2, 3, (n_rnn, D)) * 0.5
        w = np.zeros((D, n, 1))
        for o in np.nonzero(cls[k] == SAMPLE)[0]:
            w[o, rng.integers(n), 0] = rng.choice([-1.0, 1.0])
        sd[p + 'input_expand.weight'] = w
        sd[p + 'input_expand.bias'] = np.where(cls[k] == UPPER, rng.integers(-2, 3, D), 0.0)
        if top:
            w = np.zeros((D, C, 1))
            for o in np.nonzero(cls[k] == COND)[0]:
                w[o, rng.integers(C), 0] = rng.choice([-1.0, 1.0])
            sd[p + 'cond_expand.weight'] = w
            sd[p + 'cond_expand.bias'] = np.zeros(D)
            sd[p + 'spk_embedding.weight'] = rng.integers(-2, 3, (S, S)).astype(np.float64)
            w = np.zeros((D, S, 1))
            for o in np.nonzero(cls[k] == SPK)[0]:
                w[o, rng.integers(S), 0] = rng.choice([-1.0, 1.0])
            sd[p + 'spk_expand.weight'] = w
            sd[p + 'spk_expand.bias'] = np.zeros(D)
        for l in range(n_rnn):
            wih, whh = np.zeros((3 * D, D)), np.zeros((3 * D, D))
            bih, bhh = np.zeros(3 * D), rng.integers(-8, 9, 3 * D) * 0.5
            # a few small integers per W_hh row: gh stays exact and far below the gate margin
            for g in range(3 * D):
                cols = rng.choice(D, size=min(D, 6), replace=False)
                whh[g, cols] = rng.integers(-1, 2, cols.size)
            kind = rng.choice(3, size=D, p=[0.7, 0.2, 0.1])     # 0 input, 1 recurrent, 2 zero-n
            kind[:3] = (0, 1, 2)
            for u in range(D):
                for gate in range(3):
                    g = gate * D + u
                    rec = (kind[u] == 1 and gate < 2) or (kind[u] == 2 and gate == 2)
                    if rec:
                        # decided by h through W_hh; for the n gate gi_n = 0 exactly, so
                        # n = tanh(r gh_n) is +-1 where r = 1 and exactly 0 where r = 0
                        whh[g, rng.integers(D)] = rng.choice([-1.0, 1.0]) * W_REC
                        bhh[g] = rng.choice([-1.0, 1.0]) * B_REC
                        continue
                    o = rng.integers(D)
                    pw = P_SAMPLE if (l == 0 and cls[k][o] == SAMPLE) else P_INT
                    wih[g, o] = rng.choice([-1.0, 1.0]) * 2.0 ** pw
                    bih[g] = rng.choice([-1.0, 1.0]) * B_GATE
            r = p + 'rnn.'
            sd[r + 'weight_ih_l%d' % l], sd[r + 'weight_hh_l%d' % l] = wih, whh
            sd[r + 'bias_ih_l%d' % l], sd[r + 'bias_hh_l%d' % l] = bih, bhh
        # upsampling (always weight-normed): 4 entries of +-1 per input row, so ||v|| = 2 and
        # g = 2 m gives the integer weight m v exactly
        v = np.zeros((D, D, fs[k]))
        outs = np.arange(D) if k == 0 else np.nonzero(cls[k - 1] == UPPER)[0]
        for i in range(D):
            slots = rng.choice(outs.size * fs[k], size=4, replace=False)
            v[i, outs[slots // fs[k]], slots % fs[k]] = rng.choice([-1.0, 1.0], 4)
        sd[p + 'upsampling.conv_t.weight_v'] = v
        # (the bottom tier's weights are even: h in halves still gives an integer a1)
        sd[p + 'upsampling.conv_t.weight_g'] = (np.full((D, 1, 1), 4.0) if k == 0 else
                                                2.0 * rng.integers(1, 3, (D, 1, 1)))
        if k == 0:
            sd[p + 'upsampling.bias'] = -40.0 + rng.integers(-1, 2, (D, fs[k]))
        else:
            b = np.zeros((D, fs[k]))
            b[outs] = rng.integers(-1, 2, (outs.size, fs[k]))
            sd[p + 'upsampling.bias'] = b
    # the sample-level MLP: a signed permutation embedding; Tab = a thin layer of +-1 plus, per
    # unit, one tap position at which about 6 Q / D of the levels add 41..43 (a1 = relu(-40 + taps)
    # has about 6 active units, a set that moves with the history); dense W_hid and W_out
    p = 'model.sample_level_mlp.'
    perm, sgn = rng.permutation(Q), rng.choice([-1.0, 1.0], Q)
    E = np.zeros((Q, Q))
    E[np.arange(Q), perm] = sgn
    sd[p + 'embedding.weight'] = E
    FS0 = fs[0]
    u = rng.random((FS0, Q, D))
    tab = np.where(u < 0.04, -1.0, np.where(u < 0.08, 1.0, 0.0))
    n_lv = int(min(64, max(1, round(6.0 * Q / D))))
    for d in range(D):
        lv = rng.choice(Q, n_lv, replace=False)
        tab[rng.integers(FS0), lv, d] = rng.integers(41, 44, n_lv)
    # Tab[k][q][d] = sum_c E[q, c] W_in[d, c, k] = sgn[q] W_in[d, perm[q], k]
    w = np.zeros((D, Q, FS0))
    w[:, perm, :] = np.transpose(tab * sgn[None, :, None], (2, 1, 0))
    sd[p + 'input.weight'] = w
    wh = rng.integers(-1, 2, (D, D, 1)).astype(np.float64)
    sd[p + 'hidden.weight'] = wh
    # b_hid: negative, at the level that leaves about 10 units of a2 active for a typical a1
    k_act = min(D, 6)
    pre = np.stack([wh[:, rng.choice(D, k_act, replace=False), 0] @ rng.integers(1, 5, k_act)
                    for _ in range(64)])
    thr = np.quantile(pre, max(0.0, 1.0 - 10.0 / D))
    sd[p + 'hidden.bias'] = -np.floor(max(thr, 0.0)) + rng.integers(-1, 2, D)
    sd[p + 'output.weight'] = rng.integers(-1, 2, (Q, D, 1)).astype(np.float64)
    sd[p + 'output.bias'] = rng.integers(-2, 3, Q).astype(np.float64)
    return cfg, sd


def int_model(cfg, seed=1):
    """(cfg, state dict in float64) of the method A model of this config."""
    return _int_model(_key(cfg), seed)


@functools.lru_cache(maxsize=None)
def _random_model(key, seed):
    fs, D, n_rnn, C, S = key
    cfg = config(fs, D, n_rnn, C, S)
    return cfg, {k: v.astype(np.float64) for k, v in recipe.make_weights(cfg, seed).items()}


def random_model(cfg, seed):
    """(cfg, state dict in float64) of recipe.make_weights: method T."""
    return _random_model(_key(cfg), seed)


def int_cond(B, n_cond, C, seed):
    """Conditioning in quarters within [-2, 2], zeros included."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    return rng.integers(-8, 9, (B, n_cond, C)) * 0.25


def state_dict_f32(sd):
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


# ---------------------------------------------------------------------------- the reference
def _mm(a, w, order):
    """a (B, K) . w (N, K)^T, summed over k upwards or downwards."""
    if order:
        return a[:, ::-1] @ w[:, ::-1].T
    return a @ w.T


def _sigmoid(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-x))


_wcache = {}


def _weights(model, hooks):
    """The effective weights, rounded by the 'w' hook where the product stores them in T (the
    last few are kept per (model, named hook): a D = 1024 set takes seconds)."""
    key = (id(model[1]), hooks)
    if hooks in (hooks_off, hooks_bf16, hooks_weights_only):
        if key not in _wcache:
            while len(_wcache) >= 6:
                _wcache.pop(next(iter(_wcache)))
            _wcache[key] = (model[1], _weights_of(model, hooks))
        return _wcache[key][1]
    return _weights_of(model, hooks)


def _weights_of(model, hooks):
    cfg, sd = model
    fs, D, n_rnn = cfg['frame_sizes'], cfg['dim'], cfg['n_rnn']
    nt = len(fs)
    W = types.SimpleNamespace(tier=[])
    for k in range(nt):
        p = 'model.frame_level_rnns.%d.' % k
        t = types.SimpleNamespace()
        t.w_in = sd[p + 'input_expand.weight'][:, :, 0]
        t.b_in = sd[p + 'input_expand.bias']
        if k == nt - 1:
            t.w_in = np.concatenate([t.w_in, sd[p + 'cond_expand.weight'][:, :, 0]], axis=1)
            t.E = sd[p + 'spk_embedding.weight']
            t.w_s = sd[p + 'spk_expand.weight'][:, :, 0]
            t.b_row = sd[p + 'spk_expand.bias'] + sd[p + 'cond_expand.bias'] + t.b_in
        t.w_in = hooks('w', t.w_in)
        t.w_ih = [hooks('w', sd[p + 'rnn.weight_ih_l%d' % l]) for l in range(n_rnn)]
        t.w_hh = [hooks('w', sd[p + 'rnn.weight_hh_l%d' % l]) for l in range(n_rnn)]
        t.b_ih = [sd[p + 'rnn.bias_ih_l%d' % l] for l in range(n_rnn)]
        t.b_hh = [sd[p + 'rnn.bias_hh_l%d' % l] for l in range(n_rnn)]
        v, g = sd[p + 'upsampling.conv_t.weight_v'], sd[p + 'upsampling.conv_t.weight_g']
        nrm = np.sqrt((v.reshape(D, -1) ** 2).sum(1))
        wu = v * (g.reshape(-1) / nrm).reshape(D, 1, 1)               # (in, out, fs)
        t.w_up = hooks('w', np.transpose(wu, (2, 1, 0)).reshape(fs[k] * D, D))   # row j D + o
        t.b_up = np.transpose(sd[p + 'upsampling.bias'], (1, 0)).reshape(fs[k] * D)
        t.h0 = sd[p + 'h0']
        W.tier.append(t)
    p = 'model.sample_level_mlp.'
    E = hooks('w', sd[p + 'embedding.weight'])
    w_in = hooks('w', sd[p + 'input.weight'])                         # (D, Q, FS0)
    wk = np.ascontiguousarray(np.transpose(w_in, (2, 1, 0)))          # (FS0, Q, D)
    W.tab = hooks('tab', np.stack([E @ wk[k] for k in range(wk.shape[0])]))
    W.w_hid, W.b_hid = hooks('w', sd[p + 'hidden.weight'][:, :, 0]), sd[p + 'hidden.bias']
    W.w_out, W.b_out = hooks('w', sd[p + 'output.weight'][:, :, 0]), sd[p + 'output.bias']
    return W


def admits(cfg, assoc):
    """Whether the model has the association at all (the shape conditions of fold_ok / fold_top,
    whatever the dtype and the switches)."""
    fs = cfg['frame_sizes']
    if assoc == 'unfolded':
        return True
    ok = (len(fs) >= 2 and cfg['n_rnn'] == 1 and fs[0] <= 16 and fs[1] <= FOLD_MAX_FS1)
    if assoc == 'folded':
        return ok
    return ok and len(fs) == 2 and fs[0] * fs[1] + cfg['cond_dim'] <= TA_AP


def reference(model, cond, spk, noise, prefix=None, n_forced=None, state=None, assoc='unfolded',
              hooks=None, order=0, defect=None, cut=None, snaps=()):
    """Generator.__call__ in float64.

    cond (B, n_cond, C), spk (B,), noise (T, B, Q) Exp(1) draws, prefix (B, P) with n_forced (B,)
    (default P), state: None or the `.state` of an earlier call.  assoc: see ASSOCS.
    hooks(name, x): the rounding points (module docstring).  order: 0 / 1, the direction of every
    matmul's sum.
    defect: one of DEFECTS, a built-in fault (the CPU test shows the checker reports it).  cut:
    'samples' | 'upper' | 'cond' | 'spk' | 'whh' removes that influence from the tier inputs.
    Returns a namespace: seq (B, L + T) int64, logits, logp (B, T, Q), margin (B, T), gates: the
    list of (tier, layer, i, r, z, n arguments (B, D), exact-zero-n mask), state: dict(h = [tier]
    [layer] (B, D), gh0, gh1 (B, 3D) or None, hist (B, L), steps), act1 / act2 (D,): the units of
    a1 / a2 that were non-zero somewhere, snap: {frames: the state after
    that many of the call's frames} for frames in `snaps`."""
    hooks = hooks or hooks_off
    cfg, _ = model
    assert admits(cfg, assoc), assoc
    fs, D, n_rnn = cfg['frame_sizes'], cfg['dim'], cfg['n_rnn']
    nt, nfs = len(fs), recipe.cumprod(cfg['frame_sizes'])
    L, FS0 = nfs[-1], fs[0]
    W = _weights(model, hooks)
    cond = np.asarray(cond, dtype=np.float64)
    noise = np.asarray(noise, dtype=np.float64)
    B, n_cond = cond.shape[0], cond.shape[1]
    T = n_cond * L
    assert noise.shape == (T, B, Q)
    spk = np.broadcast_to(np.asarray(spk).reshape(-1), (B,))
    top = W.tier[-1]
    sp = np.roll(spk, 1) if defect == 'spk_other_row' else spk
    row_bias = top.E[sp] @ top.w_s.T + top.b_row
    if cut == 'spk':
        row_bias = np.zeros_like(row_bias)
    lut = lut2()
    seq = np.full((B, L + T), Q // 2, dtype=np.int64)
    if state is None:
        h = [[np.broadcast_to(t.h0[l], (B, D)).copy() for l in range(n_rnn)] for t in W.tier]
        steps0 = 0
    else:
        h = [[x.copy() for x in hk] for hk in state['h']]
        seq[:, :L] = state['hist']
        steps0 = state['steps']
    hold = [[x.copy() for x in hk] for hk in h]          # one tick earlier (the stale defects)
    if prefix is not None:
        prefix = np.asarray(prefix, dtype=np.int64)
        nf = np.full(B, prefix.shape[1]) if n_forced is None else np.asarray(n_forced)
    else:
        nf = np.zeros(B, dtype=np.int64)
    fold = assoc != 'unfolded'
    if fold:
        t0, t1 = W.tier[0], W.tier[1]
        Min = t0.w_ih[0] @ t0.w_in                                   # fp32 on the device
        wfold = [hooks('wfold', t0.w_ih[0] @ t1.w_up[j * D:(j + 1) * D]) for j in range(fs[1])]
        bfold = [t0.w_ih[0] @ (t1.b_up[j * D:(j + 1) * D] + t0.b_in) + t0.b_ih[0]
                 for j in range(fs[1])]
        if assoc == 'folded_top':
            min1 = hooks('min1', t1.w_ih[0] @ t1.w_in)
            P1 = row_bias @ t1.w_ih[0].T + t1.b_ih[0]
    up = [None] * nt
    G = None
    gates = []
    used = np.zeros(B, dtype=np.int64)                  # noise steps consumed ('forced_no_noise')
    logits = np.zeros((B, T, Q))
    ragged = np.arange(B) >= (B // 8) * 8
    act1, act2 = np.zeros(D, dtype=bool), np.zeros(D, dtype=bool)   # units ever non-zero

    def gru(k, l, i, gi, hp_lp, hp):
        t = W.tier[k]
        whh = np.zeros_like(t.w_hh[l]) if cut == 'whh' else t.w_hh[l]
        hsrc = hp_lp
        if defect == 'stale_h_group' and k == 0 and B > 8:
            hsrc = hp_lp.copy()
            hsrc[8:16] = hooks('h_lp', hold[k][l])[8:16]
        gh = _mm(hsrc, whh, order) + t.b_hh[l]
        ar, az = gi[:, :D] + gh[:, :D], gi[:, D:2 * D] + gh[:, D:2 * D]
        r, z = _sigmoid(ar), _sigmoid(az)
        if defect == 'bhh_n_outside':
            an = gi[:, 2 * D:] + r * (gh[:, 2 * D:] - t.b_hh[l][2 * D:]) + t.b_hh[l][2 * D:]
        else:
            an = gi[:, 2 * D:] + r * gh[:, 2 * D:]
        zero_n = (gi[:, 2 * D:] == 0) & ((r == 0) | (gh[:, 2 * D:] == 0))
        n = np.tanh(an)
        gates.append((k, l, i, ar, az, an, zero_n))
        return (hp - n) * z + n

    def state_now(hs, upto):
        gh = [None, None]
        if nt >= 2 and n_rnn == 1:
            for k in (0, 1):
                gh[k] = _mm(hooks('h_lp', hs[k][0]), W.tier[k].w_hh[0], order) + W.tier[k].b_hh[0]
        return dict(h=[[x.copy() for x in hk] for hk in hs], gh0=gh[0], gh1=gh[1],
                    hist=seq[:, upto - L:upto].copy(), steps=steps0 + upto - L)

    snap = {}
    for i in range(L, L + T):
        if i % L == 0 and i // L - 1 in snaps:
            snap[i // L - 1] = state_now(h, i)
        for k in reversed(range(nt)):
            n = nfs[k]
            if i % n:
                continue
            t = W.tier[k]
            a = lut[seq[:, i - n:i]]
            if cut == 'samples':
                a = np.zeros_like(a)
            if k == nt - 1:
                j = i // L - 1
                if defect == 'cond_frame':
                    j = min(i // L, n_cond - 1)
                cj = np.zeros_like(cond[:, j]) if cut == 'cond' else cond[:, j]
                a = np.concatenate([a, cj], axis=1)
                add = row_bias
            else:
                fi = (i // n) % fs[k + 1]
                if defect == 'fi_off_by_one':
                    fi = (fi + 1) % fs[k + 1]
                add = None if (fold and k == 0) else t.b_in + up[k + 1][:, fi]
                if cut == 'upper' and add is not None:
                    add = t.b_in + np.zeros_like(up[k + 1][:, fi])
            if defect == 'ragged_last_row' and k == 0 and ragged.any() and ragged.sum() > 1:
                a = a.copy()
                a[ragged] = a[B - 1]
            hp = [x for x in h[k]]
            if fold and k == 0:
                a = hooks('a', a)
                Gf = G[fi] if cut != 'upper' else np.broadcast_to(bfold[fi], G[fi].shape)
                gi = _mm(a, Min, order) + Gf
            elif assoc == 'folded_top' and k == 1:
                gi = _mm(hooks('atop', a), min1, order) + P1
            else:
                x = hooks('x', _mm(hooks('a', a), t.w_in, order) + add)
                gi = _mm(x, t.w_ih[0], order) + t.b_ih[0]
            for l in range(n_rnn):
                if l:
                    gi = _mm(hooks('h_lp', h[k][l - 1]), t.w_ih[l], order) + t.b_ih[l]
                hn = gru(k, l, i, gi, hooks('h_lp', hp[l]), hp[l])
                hold[k][l] = hp[l]
                h[k][l] = hn
            hl = hooks('h_lp', h[k][n_rnn - 1])
            if fold and k == 1:
                G = [_mm(hl, wfold[j], order) + bfold[j] for j in range(fs[1])]
            else:
                w_up = t.w_up
                if defect == 'upsample_order':
                    w_up = w_up.reshape(fs[k], D, D).transpose(1, 0, 2).reshape(fs[k] * D, D)
                up[k] = (_mm(hl, w_up, order) + t.b_up).reshape(B, fs[k], D)
        st = i - L
        taps = seq[:, i - FS0:i]
        if defect == 'taps_reversed':
            taps = taps[:, ::-1]
        pre = up[0][:, i % FS0].copy()
        for kk in range(FS0):
            pre += W.tab[kk][taps[:, kk]]
        a1 = hooks('a1', np.maximum(pre, 0.0))
        act1 |= (a1 > 0).any(0)
        p2 = _mm(a1, W.w_hid, order)
        if defect == 'kunit_twice' and D % 32:
            p2 = p2 + _mm(a1[:, D - D % 32:], W.w_hid[:, D - D % 32:], order)
        a2 = hooks('a2', np.maximum(p2 + W.b_hid, 0.0))
        act2 |= (a2 > 0).any(0)
        z = _mm(a2, W.w_out, order) + W.b_out
        logits[:, st] = z
        if defect == 'noise_bt':
            q = noise.reshape(B, T, Q)[:, st]
        elif defect == 'forced_no_noise':
            q = noise[np.minimum(used, T - 1), np.arange(B)]
        else:
            q = noise[st]
        sc = z - np.log(q)
        x = np.argmax(sc, axis=1)
        forced = st < nf
        if prefix is not None and st < prefix.shape[1]:
            x = np.where(forced, prefix[:, st], x)
        used += ~forced
        seq[:, i] = x
    m = logits.max(-1, keepdims=True)
    logp = logits - (m + np.log(np.exp(logits - m).sum(-1, keepdims=True)))
    sc = logits - np.log(np.transpose(noise, (1, 0, 2)))
    top2 = -np.partition(-sc, 1, axis=-1)[..., :2]
    res = types.SimpleNamespace(seq=seq, logits=logits, logp=logp, gates=gates, act1=act1,
                                act2=act2,
                                margin=top2[..., 0] - top2[..., 1])
    hs = h
    if defect == 'tick_parity' and n_cond % 2:
        # the odd last period leaves tiers with an odd tick count in the other buffer
        hs = [[hold[k][l] if (L // nfs[k]) % 2 else h[k][l] for l in range(n_rnn)]
              for k in range(nt)]
    res.state = state_now(hs, L + T)
    res.snap = snap
    return res


def part(ref, cfg, f0, n):
    """Frames [f0, f0 + n) of a run (made with snaps holding f0 + n, or ending there) as the run
    of a call that continues the state after f0 frames."""
    L = recipe.cumprod(cfg['frame_sizes'])[-1]
    T = ref.logits.shape[1]
    s0, s1 = f0 * L, (f0 + n) * L
    return types.SimpleNamespace(
        seq=ref.seq[:, s0:s1 + L], logits=ref.logits[:, s0:s1], logp=ref.logp[:, s0:s1],
        margin=ref.margin[:, s0:s1], state=ref.state if s1 == T else ref.snap[f0 + n])


def forced_margin_mask(B, T, n_forced):
    """(B, T) bool: the steps whose draw decides the stream (not forced)."""
    nf = np.zeros(B, dtype=np.int64) if n_forced is None else np.asarray(n_forced)
    return np.arange(T)[None, :] >= nf[:, None]


def pick_noise(model, cond, spk, T, B, seed0, **kw):
    """(noise, reference run) of the first of 16 consecutive seeds whose smallest margin over the
    drawn steps is >= MARGIN_MIN; AssertionError if none."""
    for s in range(seed0, seed0 + 16):
        noise = recipe.synth_noise((T, B, Q), s)
        ref = reference(model, cond, spk, noise, **kw)
        nf = kw.get('n_forced')
        if kw.get('prefix') is not None and nf is None:
            nf = np.full(B, np.asarray(kw['prefix']).shape[1])
        mask = forced_margin_mask(B, T, nf if kw.get('prefix') is not None else None)
        if not mask.any() or ref.margin[mask].min() >= MARGIN_MIN:
            return noise, ref
    raise AssertionError('no noise seed in [%d, %d) leaves every draw margin >= %g'
                         % (seed0, seed0 + 16, MARGIN_MIN))


# ---------------------------------------------------------------------------- route restatement
def fold_ok(cfg, dtype, env=None):
    """generate.hip fold_ok: dtype 'bf16' | 'fp32', env the SRNN_GEN_* switches that are off."""
    env = env or {}
    fs = cfg['frame_sizes']
    on = lambda n: env.get(n, '1') != '0'                                    # noqa: E731
    wide = cfg['dim'] % 128 == 0 if dtype == 'bf16' else (on('SRNN_GEN_FOLD_F32') and
                                                            cfg['dim'] % 64 == 0)
    return bool(wide and
                len(fs) >= 2 and cfg['n_rnn'] == 1 and fs[0] <= 16 and fs[1] <= FOLD_MAX_FS1 and
                on('SRNN_GEN_FOLD'))


def fold_top_ok(cfg, dtype, env=None):
    env = env or {}
    fs = cfg['frame_sizes']
    return bool(fold_ok(cfg, dtype, env) and len(fs) == 2 and
                fs[0] * fs[1] + cfg['cond_dim'] <= TA_AP and
                env.get('SRNN_GEN_FOLD_TOP', '1') != '0')


def tier_input_path(in_dim):
    """'tiled' | 'raised' (tiled with the LDS limit raised) | 'row' (one row per block)."""
    tlds = (64 + 8) * (in_dim | 1) * 4
    return 'row' if tlds > 160 * 1024 else 'raised' if tlds > 65536 else 'tiled'


def mlp_form(dtype, B, D, FS0, ncu=256):
    """gen_mlp_plan / pick / pick_t: None (per-sample kernels) or the name of the kernel form."""
    if FS0 < 1 or FS0 > HIST or D % 16 or D > 1024 or B < 1:
        return None
    CW = min(D, 64)
    if D % CW:
        return None
    P = D // CW
    NZ = Q // P
    if NZ % 16:
        return None
    UK = 32 if dtype == 'bf16' else 16
    NU = -(-D // UK)
    upw = -(-NU // 8)
    nzt = NZ // 16
    if -(-B // 8) * P > ncu:
        return None
    if FS0 == 16 and D == 1024:
        return 'bf16<4,4,2,1024>' if dtype == 'bf16' else 'fp32<8,4,1,1024>'
    tail = ',FS0C=16' if FS0 == 16 else ',MAXT=15' if FS0 <= 16 else ',MAXT=31'
    if upw <= 1 and nzt <= 16:
        return '<1,4,16%s>' % tail
    if upw <= 2 and nzt <= 4:
        return '<2,4,4%s>' % tail
    if upw <= 4 and nzt <= 2:
        return '<4,4,2%s>' % tail
    return None


def route(cfg, dtype, B, env=None, persistent=True):
    """What the case's table entry names: fold bits of header word 6 and whether the loop runs."""
    env = env or {}
    form = mlp_form(dtype, B, cfg['dim'], cfg['frame_sizes'][0])
    loop = form is not None and persistent and env.get('SRNN_GEN_PERSIST', '1') != '0'
    nfs = recipe.cumprod(cfg['frame_sizes'])
    return types.SimpleNamespace(
        fold=fold_ok(cfg, dtype, env), fold_top=fold_top_ok(cfg, dtype, env), form=form, loop=loop,
        inputs=[tier_input_path(n + (cfg['cond_dim'] if k == len(nfs) - 1 else 0))
                for k, n in enumerate(nfs)])


def assoc_of(r):
    return 'folded_top' if r.fold_top else 'folded' if r.fold else 'unfolded'


# ---------------------------------------------------------------------------- checkers
def parse_state(blob, cfg, fold):
    """The records of a GenState blob ((B, row_bytes) uint8 ndarray) as a dict of arrays."""
    fs, D, n_rnn = cfg['frame_sizes'], cfg['dim'], cfg['n_rnn']
    L, nh = recipe.cumprod(fs)[-1], len(fs) * n_rnn
    w = np.ascontiguousarray(blob).view(np.uint32)
    o = 16 + L
    out = dict(hdr=w[:, :8].copy(), steps=w[:, 8:10].copy().view(np.int64)[:, 0],
               hist=w[:, 16:o].astype(np.int64),
               h=w[:, o:o + nh * D].copy().view(np.float32).reshape(-1, nh, D))
    o += nh * D
    if fold:
        out['gh0'] = w[:, o:o + 3 * D].copy().view(np.float32)
        out['gh1'] = w[:, o + 3 * D:o + 6 * D].copy().view(np.float32)
    return out


def _report(name, bad, got, ref, names):
    idx = np.argwhere(bad)
    msgs = []
    for ix in idx[:6]:
        ix = tuple(ix)
        msgs.append('%s[%s] got %r ref %r' % (name, ', '.join('%s %d' % (n, v)
                                                             for n, v in zip(names, ix)),
                                              got[ix].item(), ref[ix].item()))
    return ['%s: %d of %d differ: %s' % (name, len(idx), bad.size, '; '.join(msgs))]


def check_stream(seq, ref):
    """seq (B, L + T), prefix columns included, against the reference, by (row, column)."""
    seq = np.asarray(seq)
    if seq.shape != ref.seq.shape:
        return ['seq: shape %s, reference %s' % (seq.shape, ref.seq.shape)]
    bad = seq != ref.seq
    return _report('seq', bad, seq, ref.seq, ('row', 'column')) if bad.any() else []


def logp_units(logp, ref):
    """(|got - ref| - ulp32(ref) / 2) / 2^-24 per element: what C_LSE has to cover."""
    got = np.asarray(logp, dtype=np.float64)
    return (np.abs(got - ref.logp) - 0.5 * ulp32(ref.logp)) * 2.0 ** 24


def check_logp(logp, ref, c_lse):
    assert c_lse <= 64, 'C_LSE above 64 is refused'
    u = logp_units(logp, ref)
    bad = ~(u <= c_lse)
    return (_report('logp', bad, np.asarray(logp, dtype=np.float64), ref.logp,
                    ('row', 'step', 'level')) if bad.any() else [])


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32) + np.float32(0.0)).view(np.int32)


def check_state(rec, ref, cfg, dtype, fold_bits, steps=None):
    """A parsed record against the reference's final state: header, step count, history, every h
    and the carried gh blocks bit for bit (-0.0 read as +0.0)."""
    fs, D, n_rnn = cfg['frame_sizes'], cfg['dim'], cfg['n_rnn']
    L = recipe.cumprod(fs)[-1]
    st = ref.state
    out = []
    want = np.array([0x314E5253, 1 if dtype == 'bf16' else 0, len(fs), n_rnn, D, L, fold_bits, 0],
                    dtype=np.uint32)
    bad = rec['hdr'] != want            # (word 1: SrnnDtype, fp32 = 0, bf16 = 1)
    if bad.any():
        out += _report('header', bad, rec['hdr'], np.broadcast_to(want, bad.shape),
                       ('row', 'word'))
    want_steps = np.full(rec['steps'].shape, st['steps'] if steps is None else steps)
    if (rec['steps'] != want_steps).any():
        out += _report('steps', rec['steps'] != want_steps, rec['steps'], want_steps, ('row',))
    if (rec['hist'] != st['hist']).any():
        out += _report('history', rec['hist'] != st['hist'], rec['hist'], st['hist'],
                       ('row', 'column'))
    for k in range(len(fs)):
        for l in range(n_rnn):
            g, r = _bits(rec['h'][:, k * n_rnn + l]), _bits(st['h'][k][l])
            if (g != r).any():
                out += _report('h[tier %d layer %d]' % (k, l), g != r, rec['h'][:, k * n_rnn + l],
                               st['h'][k][l], ('row', 'unit'))
    if fold_bits & 1:
        for name in ('gh0', 'gh1'):
            g, r = _bits(rec[name]), _bits(st[name])
            if (g != r).any():
                out += _report(name, g != r, rec[name], st[name], ('row', 'unit'))
    return out


def check_case(got_seq, got_logp, rec, ref, cfg, dtype, fold_bits, c_lse):
    out = check_stream(got_seq, ref)
    if got_logp is not None:
        out += check_logp(got_logp, ref, c_lse)
    if rec is not None:
        out += check_state(rec, ref, cfg, dtype, fold_bits)
    return out


def reference_as_result(ref, cfg, fold):
    """A reference run dressed as a device result (seq, logp in fp32, parsed record): what the
    CPU test feeds the checker, with a defect built into `ref`."""
    D, n_rnn = cfg['dim'], cfg['n_rnn']
    st = ref.state
    B = ref.seq.shape[0]
    rec = dict(hdr=np.zeros((B, 8), dtype=np.uint32), steps=np.full(B, st['steps']),
               hist=st['hist'],
               h=np.stack([st['h'][k][l] for k in range(len(st['h'])) for l in range(n_rnn)],
                          axis=1).astype(np.float32))
    if fold:
        rec['gh0'], rec['gh1'] = st['gh0'].astype(np.float32), st['gh1'].astype(np.float32)
    return ref.seq, ref.logp.astype(np.float32), rec


# ---------------------------------------------------------------------------- proofs (CPU)
def gate_margin(ref):
    """The smallest |argument| over every r, z and non-zero n gate of a run, and whether every
    zero n came from exact zeros."""
    lo = np.inf
    for _, _, _, ar, az, an, zero_n in ref.gates:
        lo = min(lo, np.abs(ar).min(), np.abs(az).min())
        nz = an != 0
        if nz.any():
            lo = min(lo, np.abs(an[nz]).min())
        if (~nz & ~zero_n).any():
            return 0.0
    return lo


def stored_values(model, cond, spk, noise, **kw):
    """Every value a bf16 run stores in bf16 and every fp32 value compared bit for bit, gathered
    by running the reference with a recording hook."""
    seen = []

    def rec(name, x):
        if name not in ('a', 'atop', 'x', 'wfold', 'min1'):      # those feed saturated gates only
            seen.append((name, np.asarray(x)))
        return x
    ref = reference(model, cond, spk, noise, hooks=rec, **kw)
    return seen, ref


# ---------------------------------------------------------------------------- the tables
class Case(types.SimpleNamespace):
    @property
    def id(self):
        e = ','.join('%s=%s' % (k.replace('SRNN_GEN_', ''), v) for k, v in sorted(self.env.items()))
        return '-'.join(str(x) for x in (
            'x'.join(map(str, self.fs)) + ('r%d' % self.n_rnn if self.n_rnn > 1 else '') +
            ('c%d' % self.cond_dim if self.cond_dim != 6 else ''),
            'D%d' % self.D, self.dtype, 'B%d' % self.B, 'n%d' % self.n_cond, 'ct%d' % self.level,
            ('g' if self.graph else 'e') + ('' if self.persistent else 'ps'),
            self.forced or 'free', e or 'dflt'))

    @property
    def cfg(self):
        return config(self.fs, self.D, self.n_rnn, self.cond_dim)


def case(fs, D, dtype, B=9, n_cond=2, level=0, graph=True, persistent=True, env=None, forced=None,
         n_rnn=1, cond_dim=6):
    return Case(fs=tuple(fs), D=D, dtype=dtype, B=B, n_cond=n_cond, level=level, graph=graph,
                persistent=persistent, env=dict(env or {}), forced=forced, n_rnn=n_rnn,
                cond_dim=cond_dim)


MODELS = [((4,), {}), ((4, 2), {}), ((16, 2), {}), ((16, 3), {}), ((4, 2, 2), {}), ((20, 2), {}),
          ((32, 2), {}), ((2, 9), {}), ((4, 2), dict(n_rnn=2)), ((16, 4), dict(cond_dim=86)),
          ((4, 2), dict(cond_dim=224)), ((4, 2), dict(cond_dim=570))]
SWITCHES = ('SRNN_GEN_LOCAL', 'SRNN_GEN_FOLD', 'SRNN_GEN_FOLD_F32', 'SRNN_GEN_FOLD_TOP',
            'SRNN_GEN_FUSE_GATES', 'SRNN_GEN_NOISE_AHEAD', 'SRNN_GEN_WFRAG', 'SRNN_GEN_TICK_GEMM')
DT = ('fp32', 'bf16')


def table_a():
    t = []
    # every model at D = 64, both dtypes, ragged batch, block + odd block
    for fs, kw in MODELS:
        t += [case(fs, 64, dt, 9, 3, **kw) for dt in DT]
        # (bf16 folds at dim % 128 == 0 only: the models that admit a fold, at D = 128 as well)
        if admits(config(fs, 128, **kw), 'folded'):
            t += [case(fs, 128, 'bf16', 9, 3, **kw)]
    # odd FS1 with n_cond 2, 3, 5
    t += [case((16, 3), 64, dt, 9, n) for dt in DT for n in (2, 5)]
    # widths (D = 80: the plan declines; 1024: the compiled shapes, FS0 = 4: fp32 declined)
    for D in (16, 48, 128, 256, 512, 80):
        t += [case((16, 2), D, dt, 9, 2) for dt in DT] + [case((4, 2), D, dt, 9, 2) for dt in DT]
    t += [case((20, 2), D, dt, 9, 1) for D in (16, 256, 512) for dt in DT]
    t += [case((16, 2), 1024, dt, 9, 2) for dt in DT] + [case((4, 2), 1024, dt, 9, 1) for dt in DT]
    # control levels at default controls, every form and dtype
    for lv in (1, 2):
        t += [case((16, 2), D, dt, 9, 1, level=lv) for D in (64, 256, 512) for dt in DT]
        t += [case((4, 2), D, dt, 9, 1, level=lv) for D in (64, 256, 512) for dt in DT]
        t += [case((20, 2), D, dt, 9, 1, level=lv) for D in (64, 256, 512) for dt in DT]
        t += [case((16, 2), 1024, dt, 9, 1, level=lv) for dt in DT]
        t += [case((4, 2), 1024, 'bf16', 9, 1, level=lv)]
    # batch
    # (12: a ragged group of more than one row)
    t += [case((16, 2), 64, dt, B, 2) for B in (1, 8, 12, 17) for dt in DT]
    t += [case((4, 2, 2), 128, 'bf16', B, 2) for B in (1, 8, 17)]
    # n_cond: odd block alone, block, block + odd, eager + captured + replay + odd, two replays
    t += [case((4, 2), 64, dt, 9, n) for n in (1, 2) for dt in DT]
    t += [case((4, 2), 64, dt, 9, n, graph=g) for n in (5, 7) for g in (True, False) for dt in DT]
    t += [case((16, 2), 64, 'bf16', 9, n, graph=g) for n in (5, 7) for g in (True, False)]
    # (bf16 folds at dim % 128 == 0 only: the folded bf16 ticks, fold_top and the D = 1024 in-launch
    #  tick GEMM through the same sequences of blocks)
    t += [case((16, 2), D, 'bf16', 9, n, graph=g) for D in (128, 1024) for n in (5, 7)
          for g in (True, False)]
    # paths: one thing changed, at D = 64 and one at D = 1024
    t += [case((16, 2), 64, dt, 9, 3, persistent=False) for dt in DT]
    t += [case((16, 2), 1024, 'bf16', 9, 1, persistent=False)]
    for sw in SWITCHES:
        t += [case((16, 2), 64, dt, 9, 3, env={sw: '0'}) for dt in DT]
        t += [case(fs, 128, 'bf16', 9, 3, env={sw: '0'}) for fs in ((16, 2), (4, 2, 2))]
        t += [case((16, 2), 1024, 'bf16', 9, 2, env={sw: '0'})]
    # forced prefix along a stream that is not the model's own
    t += [case(fs, 64, dt, 9, 2, forced='mixed') for fs in ((16, 2), (4, 2, 2)) for dt in DT]
    t += [case((16, 2), 128, 'bf16', 9, 2, forced='mixed')]
    t += [case((16, 2), 1024, 'bf16', 9, 2, forced='mixed'),
          case((16, 2), 64, 'bf16', 9, 2, forced='mixed', persistent=False),
          case((16, 2), 64, 'fp32', 9, 2, forced='mixed', level=1)]
    seen, out = set(), []
    for c in t:
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)
    return out


# the same run as one call, as calls over n_cond splits 1 | 2 | 2 and through a session's chunks
CARRY = [case(fs, D, dt, 9, 5) for fs, D in (((16, 2), 64), ((16, 3), 64), ((4, 2, 2), 64),
                                             ((16, 3), 128), ((16, 2), 1024)) for dt in DT
         if not (D == 1024 and dt == 'fp32') and not (D == 128 and dt == 'fp32')]
SPLITS = (1, 2, 2)


def forced_lengths(c):
    """Per-row forced lengths 0, 1, FS0 - 1, FS0, FS0 + 1, L, T (cycled over the rows)."""
    L = int(np.prod(c.fs))
    T = c.n_cond * L
    v = [0, 1, c.fs[0] - 1, c.fs[0], c.fs[0] + 1, L, T]
    return np.array([v[b % len(v)] for b in range(c.B)], dtype=np.int64)


def inputs(c, model_seed=1):
    """(model, cond, spk, noise, prefix, n_forced, reference run) of a method A case: the
    reference does not depend on the dtype, the association or the path (test_cpu proves it), so
    it is computed once per (model, B, n_cond, forced)."""
    return _inputs(_key(c.cfg), c.B, c.n_cond, c.forced, model_seed)


@functools.lru_cache(maxsize=None)
def _inputs(key, B, n_cond, forced, model_seed):
    fs, D, n_rnn, C, S = key
    cfg = config(fs, D, n_rnn, C, S)
    model = int_model(cfg, model_seed)
    L = int(np.prod(fs))
    T = n_cond * L
    cond = int_cond(B, n_cond, C, B + 10 * n_cond)
    spk = np.arange(B) % S
    prefix = n_forced = None
    if forced:
        rng = np.random.Generator(np.random.PCG64(77 + B + T))
        prefix = rng.integers(0, Q, (B, T))
        n_forced = forced_lengths(types.SimpleNamespace(fs=fs, n_cond=n_cond, B=B))
    for _ in range(8):
        noise, ref = pick_noise(model, cond, spk, T, B, 100 * n_cond + B, prefix=prefix,
                                n_forced=n_forced, snaps=tuple(np.cumsum(SPLITS)))
        if not forced:
            break
        # every forced value differs from the draw the run would have made at that step
        draw = np.argmax(ref.logits - np.log(np.transpose(noise, (1, 0, 2)).astype(np.float64)), -1)
        same = (prefix == draw) & ~forced_margin_mask(B, T, n_forced)
        if not same.any():
            break
        prefix = np.where(same, (prefix + 1) % Q, prefix)
    else:
        raise AssertionError('forced prefix keeps meeting the run\'s own draws')
    return model, cond, spk, noise, prefix, n_forced, ref


# ---------------------------------------------------------------------------- method T
# C_LSE: what the device's 256 expf terms, wave sum and logf may add to 0.5 ulp32 of the exact
# log-prob, in units of 2^-24: the largest value over every method A case on the MI355X is 9.12,
# doubled and rounded up
C_LSE = 19


def case_t(fs, D, dtype, path, seed=5, B=9, n_cond=2, n_rnn=1, env=None):
    """path: 'loop' (the default route), 'unfolded' (SRNN_GEN_FOLD=0), 'sample' (per-sample
    kernels)."""
    env = dict(env or {})
    if path == 'unfolded':
        env['SRNN_GEN_FOLD'] = '0'
    c = case(fs, D, dtype, B, n_cond, persistent=path != 'sample', env=env, forced='all',
             n_rnn=n_rnn, cond_dim=43)
    c.seed = seed
    c.assoc = assoc_of(route(c.cfg, dtype, B, env, c.persistent))
    return c


def table_t():
    t = []
    for fs, D in (((16, 4), 64), ((16, 4), 128), ((4, 2, 2), 64)):
        t += [case_t(fs, D, dt, p) for dt in DT for p in ('loop', 'unfolded', 'sample')]
    t += [case_t((20, 4), 32, dt, p, n_rnn=2) for dt in DT for p in ('loop', 'sample')]
    t += [case_t((16, 4), 1024, 'fp32', p) for p in ('loop', 'unfolded', 'sample')]
    t += [case_t((16, 4), 1024, 'bf16', p) for p in ('loop', 'unfolded', 'sample')]
    t += [case_t((16, 4), 1024, 'bf16', 'loop', env={'SRNN_GEN_TICK_GEMM': '0'})]
    return t


TABLE_T = table_t()


def oracle_run(model, cond, spk, noise, prefix):
    """The project's CPU fp32 oracle along the forced stream: (logp (B, T, Q), h[tier][layer])."""
    import torch
    import samplernn_oracle as O
    import stream_ref
    cfg, sd = model
    orc = O.from_state_dict(cfg, state_dict_f32(sd))
    B = cond.shape[0]
    _, lp, _, st = stream_ref.generate(orc, B, torch.from_numpy(cond).float(), spk,
                                       torch.from_numpy(noise), prefix=prefix)
    return lp.numpy().astype(np.float64), [[h[l].numpy().astype(np.float64)
                                            for l in range(cfg['n_rnn'])] for h in st[0]]


def _hdev(a, b):
    return max(np.abs(x - y).max() for p, q in zip(a, b) for x, y in zip(p, q))


def inputs_t(c):
    """(model, cond, spk, noise, prefix, reference run, bounds) of a method T case."""
    return _inputs_t(_key(c.cfg), c.B, c.n_cond, c.seed, c.dtype, c.assoc)


@functools.lru_cache(maxsize=None)
def _inputs_t(key, B, n_cond, seed, dtype, assoc):
    fs, D, n_rnn, C, S = key
    cfg = dict(config(fs, D, n_rnn, C, S), spk_dim=6)
    model = random_model(cfg, seed)
    L = int(np.prod(fs))
    T = n_cond * L
    cond = recipe.synth_cond((B, n_cond, C), seed + 1)
    spk = np.arange(B) % cfg['spk_dim']
    noise = recipe.synth_noise((T, B, Q), seed + 2)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    # a stream that is not the model's own: a slow walk with jumps, every step forced
    prefix = (128 + np.cumsum(rng.integers(-6, 7, (B, T)), axis=1) +
              np.where(rng.random((B, T)) < 0.05, rng.integers(-100, 100, (B, T)), 0)) % Q
    bound = types.SimpleNamespace()
    if dtype == 'fp32':
        ref = reference(model, cond, spk, noise, prefix=prefix)
        olp, oh = oracle_run(model, cond, spk, noise, prefix)
        bound.e_lp, bound.e_h = np.abs(olp - ref.logp).max(), _hdev(oh, ref.state['h'])
        bound.lp_max, bound.lp_mean, bound.h_max = 4 * bound.e_lp, np.inf, 4 * bound.e_h
    else:
        ref = reference(model, cond, spk, noise, prefix=prefix, assoc=assoc, hooks=hooks_bf16)
        off = reference(model, cond, spk, noise, prefix=prefix, assoc=assoc,
                        hooks=hooks_weights_only)
        d = np.abs(off.logp - ref.logp)
        bound.e_lp, bound.e_mean = d.max(), d.mean()
        bound.e_h = _hdev(off.state['h'], ref.state['h'])
        bound.lp_max, bound.lp_mean, bound.h_max = 2 * bound.e_lp, 2 * bound.e_mean, 2 * bound.e_h
    return model, cond, spk, noise, prefix, ref, bound
