"""Exact-arithmetic GEMM cases: the builder and the checker of the conformance sweep.

The method.  A and B hold integers in [-3, 3] (exact in bf16) and K <= 8192, so every product
and every partial sum is an integer below 2^17: whatever the order of accumulation (MFMA,
split-K partials, atomics, a library), the fp32 sum is the same bits.  alpha, beta, Cin and
the bias are dyadic fractions (alpha in {1, 1.5, -0.5}, beta in {0, 0.5, 1}, Cin in quarters
within +-16, bias in quarters within +-8), so alpha * acc + beta * Cin + bias is a multiple of
1/8 below 2^20: it needs 23 bits and is exact in fp32 with or without fused multiply-adds.
An fp32 output must therefore equal the float64 reference bit for bit, and a bf16 output its
round-to-nearest-even.  There is no tolerance anywhere.

One equivalence is applied before the bits are compared: -0.0 is read as +0.0.  alpha = -0.5
on a zero sum gives -0.0, a memset-then-atomics split-K gives +0.0, and fmaxf(-0.0, 0.0) may
return either; the sign of an exact zero is not part of the GEMM's contract.

Placement.  Every operand is a window inside a larger buffer whose every other element holds
a canary (one fixed quiet-NaN pattern): guard rows before and after, row padding, batch
padding.  A stray read poisons the output, a stray write changes a canary.

Plain helper module (no fixtures): the CPU test proves the cases, the GPU test runs them.
"""
import dataclasses
import types

import torch

CANARY32 = 0x7FC12345          # a quiet NaN as fp32 (and the filler of int32 views)
CANARY16 = 0x7FC1              # its upper half: a quiet NaN as bf16 (and the int16 filler)
GUARD_ROWS = 2

# name -> (extra elements per row, front offset in elements past a 16-byte boundary)
PLACEMENTS = {'tight': (0, 0), 'pad8': (8, 0), 'pad1': (1, 0), 'off1': (0, 1)}
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}

INELIGIBLE = {6: 'not eligible for the thin path', 4: 'not eligible for the skinny path',
              5: 'not eligible for the gemm3 path', 3: 'not eligible for the gemm2 path'}

# epilogues by name (fields of Case)
EPI = {
    'plain': {},
    'alpha': dict(alpha=1.5),
    'cbias': dict(bias=1),
    'rbias': dict(bias=2),
    'cin': dict(cin=True, beta=0.5),
    'cin1': dict(cin=True, beta=1.0, alpha=-0.5),
    'relu': dict(relu=True, alpha=-0.5),
    'cbrelu': dict(bias=1, relu=True),
    'mask': dict(mask=True),
    'beta0': dict(cin=True, beta=0.0),                       # Cin given, all canary, unread
    'epi': dict(alpha=1.5, beta=0.5, cin=True, bias=1, relu=True),            # no mask
    'full': dict(alpha=1.5, beta=0.5, cin=True, bias=1, relu=True, mask=True),
    'fullr': dict(alpha=-0.5, beta=1.0, cin=True, bias=2, relu=True, mask=True),
}


@dataclasses.dataclass(frozen=True)
class Case:
    tile: int                   # forced backend code, -1: the router chooses
    dtype: str                  # 'f32' / 'bf16' (A, B, mask)
    out: str                    # 'f32' / 'bf16'
    layout: str                 # 'NN' 'NT' 'TN' 'TT' (op(A), op(B))
    M: int
    N: int
    K: int
    place: str = 'tight'        # placement of every operand ...
    places: tuple = ()          # ... but these: (('C', 'pad1'), ...)
    epi: str = 'plain'
    expect: str = 'takes'       # 'takes' / 'refuses'
    batch: int = 1
    shared: str = ''            # 'A' / 'B': that operand's batch stride is 0 (one for all)
    sc_extra: int = 0           # sC = M * ldc + sc_extra
    bits: str = ''              # 'in': mask as bits; 'out': bits of the output wanted
    env: tuple = ()             # (('SRNN_...', '0'), ...) set for the call
    blaslt: object = None       # expected rise of srnn_blaslt_calls(), None: not looked at
    alpha: float = 1.0
    beta: float = 0.0
    cin: bool = False
    bias: int = 0               # 0 none, 1 per column, 2 per row
    relu: bool = False
    mask: bool = False

    def placement(self, operand):
        return dict(self.places).get(operand, self.place)

    @property
    def id(self):
        s = 't%d-%s>%s-%s-%dx%dx%d-%s-%s' % (self.tile, self.dtype, self.out, self.layout,
                                              self.M, self.N, self.K, self.place, self.epi)
        for k, v in self.places:
            s += '-%s.%s' % (k, v)
        if self.batch > 1:
            s += '-b%d%s%s' % (self.batch, 's%s0' % self.shared if self.shared else '',
                               '+%d' % self.sc_extra if self.sc_extra else '')
        if self.bits:
            s += '-bits_' + self.bits
        for k, v in self.env:
            s += '-%s=%s' % (k.replace('SRNN_', ''), v)
        if self.expect != 'takes':
            s += '-' + self.expect
        return s


def case(tile, dtype, out, layout, M, N, K, place='tight', epi='plain', expect='takes', **kw):
    """A Case with the named epilogue's fields filled in."""
    places = tuple(sorted(kw.pop('places', {}).items()))
    env = tuple(sorted(kw.pop('env', {}).items()))
    return Case(tile, dtype, out, layout, M, N, K, place=place, places=places, epi=epi,
                expect=expect, env=env, **dict(EPI[epi], **kw))


def _esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _ints(t):
    """The bits of a floating (or integer) tensor as integers of the same width."""
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _canary(dtype):
    return CANARY32 if _esize(dtype) == 4 else CANARY16


class Window:
    """`batch` windows of rows x cols elements, rows `ld` apart and windows `stride` apart
    (0: one shared window), `front` elements into a canary-filled 1-D buffer."""

    def __init__(self, dtype, rows, cols, place, device, batch=1, shared=False, extra=0,
                 ld=None):
        pad, off = PLACEMENTS[place]
        self.dtype, self.rows, self.cols, self.place = dtype, rows, cols, place
        self.ld = max(cols, 1) + pad if ld is None else ld
        self.nb = 1 if shared else batch
        self.stride = 0 if shared or batch == 1 else rows * self.ld + extra
        al = 16 // _esize(dtype)                                 # elements per 16 bytes
        guard = -(-GUARD_ROWS * self.ld // al) * al
        self.front = guard + off
        span = (self.nb - 1) * self.stride + max(rows, 1) * self.ld
        self.buf = torch.empty(self.front + span + guard + al, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        _ints(self.buf).fill_(_canary(dtype))
        b = torch.arange(self.nb).view(-1, 1, 1) * self.stride
        r = torch.arange(rows).view(1, -1, 1) * self.ld
        self.index = (self.front + b + r + torch.arange(cols).view(1, 1, -1)).reshape(-1)
        self.before = None

    def fill(self, values):
        """values: (nb, rows, cols), any dtype exact in this window's."""
        self.buf[self.index.to(self.buf.device)] = values.reshape(-1).to(self.buf)

    def read(self):
        return self.buf[self.index.to(self.buf.device)].view(self.nb, self.rows, self.cols)

    def view(self):
        """The first window as a 2-D strided view (never empty, so it keeps its pointer)."""
        return self.buf.as_strided((max(self.rows, 1), max(self.cols, 1)), (self.ld, 1),
                                   self.front)

    def misalignment(self):
        """Bytes of the window's base pointer past a 16-byte boundary."""
        return self.view().data_ptr() % 16

    def snapshot(self):
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(_ints(self.buf), _ints(self.before))

    def outside_ok(self):
        """Every element outside the windows still holds the canary."""
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        keep[self.index.to(self.buf.device)] = False
        return bool((_ints(self.buf)[keep] == _canary(self.dtype)).all())


def _draw(gen, shape, lo, hi, step=1.0):
    return torch.randint(lo, hi + 1, shape, generator=gen).double() * step


def _reference(c, A, B, cin, bias, mask, dtype=torch.float64):
    """act(alpha op(A) op(B) + beta Cin + bias) where mask > 0, else 0; (batch, M, N) in
    `dtype`, every operation in that dtype.  A: (nb, M, K) and B: (nb, K, N) already as op()."""
    A, B = A.to(dtype), B.to(dtype)
    v = c.alpha * torch.matmul(A, B).expand(c.batch, c.M, c.N)
    if c.beta != 0.0:
        v = v + c.beta * cin.to(dtype)
    if c.bias == 1:
        v = v + bias.to(dtype).view(1, 1, c.N)
    elif c.bias == 2:
        v = v + bias.to(dtype).view(1, c.M, 1)
    if c.relu:
        v = v.clamp_min(0.0)
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros((), dtype=dtype))
    return v


def build(c, device='cpu', seed=None):
    """Place a case's operands on `device` and compute its reference (on the CPU)."""
    assert c.K <= 8192 and c.layout in ('NN', 'NT', 'TN', 'TT') and c.expect in ('takes', 'refuses')
    assert c.alpha in (1.0, 1.5, -0.5) and c.beta in (0.0, 0.5, 1.0)
    gen = torch.Generator().manual_seed(
        c.M * 1000003 + c.N * 1009 + c.K * 17 + ('NN', 'NT', 'TN', 'TT').index(c.layout)
        if seed is None else seed)
    dt, do = DTYPES[c.dtype], DTYPES[c.out]
    tA, tB = c.layout[0] == 'T', c.layout[1] == 'T'
    M, N, K, nb = c.M, c.N, c.K, c.batch
    t = types.SimpleNamespace(case=c, device=device)
    # values, as op(A) (nb or 1, M, K) and op(B) (nb or 1, K, N)
    A = _draw(gen, (1 if c.shared == 'A' else nb, M, K), -3, 3)
    B = _draw(gen, (1 if c.shared == 'B' else nb, K, N), -3, 3)
    cin = _draw(gen, (nb, M, N), -64, 64, 0.25) if c.cin else None
    bias = _draw(gen, (N if c.bias == 1 else M,), -32, 32, 0.25) if c.bias else None
    mask = _draw(gen, (nb, M, N), -1, 1) if (c.mask or c.bits == 'in') else None
    # the exactness precondition, elementwise in float64
    bound = abs(c.alpha) * torch.matmul(A.abs(), B.abs()).expand(nb, M, N)
    if cin is not None:
        bound = bound + (c.beta * cin).abs()
    if c.bias:
        bound = bound + (bias.abs().view(1, 1, N) if c.bias == 1 else bias.abs().view(1, M, 1))
    assert bound.numel() == 0 or float(bound.max()) < 2.0 ** 20, 'case %s is not exact' % c.id
    t.values = dict(A=A, B=B, cin=cin, bias=bias, mask=mask)
    t.ref = _reference(c, A, B, cin, bias, mask)
    # windows
    w = {}
    w['A'] = Window(dt, K if tA else M, M if tA else K, c.placement('A'), device, nb,
                    shared=c.shared == 'A')
    w['A'].fill(A.transpose(1, 2) if tA else A)
    w['B'] = Window(dt, N if tB else K, K if tB else N, c.placement('B'), device, nb,
                    shared=c.shared == 'B')
    w['B'].fill(B.transpose(1, 2) if tB else B)
    w['C'] = Window(do, M, N, c.placement('C'), device, nb, extra=c.sc_extra)
    if c.cin:
        w['Cin'] = Window(torch.float32, M, N, c.placement('Cin'), device, nb)
        if c.beta != 0.0:                     # beta == 0: the window stays canary too
            w['Cin'].fill(cin)
    if c.bias:
        w['bias'] = Window(torch.float32, 1, bias.numel(), c.placement('bias'), device)
        w['bias'].fill(bias.view(1, 1, -1))
    if c.mask:
        # a batched mask lies as C does: batch stride sC, its own row stride
        ldm = N + PLACEMENTS[c.placement('mask')][0]
        assert nb == 1 or w['C'].stride >= M * ldm
        w['mask'] = Window(dt, M, N, c.placement('mask'), device, nb,
                           extra=w['C'].stride - M * ldm if nb > 1 else 0)
        w['mask'].fill(mask)
    ng = (N + 15) // 16
    if c.bits == 'in':
        # row-major bits, bit c % 16 of word [row][c / 16] = (mask > 0), rows 4 words padded
        w['mbi'] = Window(torch.int16, M, ng, 'tight', device, ld=-(-ng // 4) * 4 + 4)
        w['mbi'].fill(pack_bits(mask[0] > 0))
    if c.bits == 'out':
        w['mbo'] = Window(torch.int16, M, ng, 'tight', device, ld=-(-ng // 4) * 4 + 4)
    t.w = w
    for k, x in w.items():
        if k not in ('C', 'mbo'):
            x.snapshot()
    return t


def pack_bits(pos):
    """(M, N) bool -> (1, M, ceil(N / 16)) int16 words, bit c % 16 of word c / 16."""
    M, N = pos.shape
    ng = (N + 15) // 16
    p = torch.zeros((M, ng * 16), dtype=torch.int64)
    p[:, :N] = pos.to(torch.int64)
    words = (p.view(M, ng, 16) << torch.arange(16)).sum(-1)
    words = torch.where(words >= 32768, words - 65536, words)
    return words.to(torch.int16).view(1, M, ng)


def expected_bits(t):
    """The reference cast to the case's output dtype, as integers, -0.0 read as +0.0."""
    return _ints((t.ref.to(torch.float32) + 0.0).to(DTYPES[t.case.out]) + 0.0)


def gemm_kwargs(t):
    """Keyword arguments of samplernn_hip.gemm for the built case."""
    c, w = t.case, t.w
    kw = dict(transA=c.layout[0] == 'T', transB=c.layout[1] == 'T', out=w['C'].view(),
              alpha=c.alpha, beta=c.beta, relu=c.relu, M=c.M, N=c.N, K=c.K, lda=w['A'].ld,
              ldb=w['B'].ld, ldc=w['C'].ld, batch=c.batch, sA=w['A'].stride, sB=w['B'].stride,
              sC=w['C'].stride, tile=c.tile)
    if c.cin:
        kw.update(cin=w['Cin'].view(), ldcin=w['Cin'].ld, sCin=w['Cin'].stride)
    if c.bias:
        kw.update(bias=w['bias'].view(), bias_mode=c.bias)
    if c.mask:
        kw.update(mask=w['mask'].view())
    if c.bits == 'in':
        kw.update(mask_bits=w['mbi'].view())
    if c.bits == 'out':
        kw.update(bits_out=w['mbo'].view())
    return w['A'].view(), w['B'].view(), kw


def evaluate_f32(t):
    """The case evaluated in float32 on the CPU from the placed operands (read back out of
    their windows), written into the C window: what an exact kernel leaves behind."""
    c, w = t.case, t.w
    A, B = w['A'].read().cpu().float(), w['B'].read().cpu().float()
    A = A.transpose(1, 2) if c.layout[0] == 'T' else A
    B = B.transpose(1, 2) if c.layout[1] == 'T' else B
    cin = w['Cin'].read().cpu() if c.cin and c.beta != 0.0 else None
    bias = w['bias'].read().cpu().view(-1) if c.bias else None
    mask = w['mask'].read().cpu().float() if c.mask else None
    if c.bits == 'in':
        words = w['mbi'].read().cpu().view(c.M, -1).to(torch.int64) & 0xffff
        cols = torch.arange(c.N)
        mask = ((words[:, cols // 16] >> (cols % 16)) & 1).float().view(1, c.M, c.N)
    v = _reference(c, A, B, cin, bias, mask, dtype=torch.float32)
    w['C'].fill(v.to(DTYPES[c.out]))
    if c.bits == 'out':
        w['mbo'].fill(pack_bits(v[0].to(DTYPES[c.out]).float() > 0))
    return v


def check(t):
    """None when the built case's buffers hold an exact result, else the report: first bad
    (batch, row, col), how many differ, and whether the damage is inside or outside a window."""
    c, w = t.case, t.w
    bad = []
    got = _ints(w['C'].read().cpu() + 0.0)
    want = expected_bits(t)
    diff = (got != want)
    if bool(diff.any()):
        b, r, col = (int(x) for x in diff.nonzero()[0])
        bad.append('inside the C window: %d of %d elements differ, first at (batch %d, row %d, '
                   'col %d): got 0x%x, want 0x%x' % (int(diff.sum()), diff.numel(), b, r, col,
                                                     int(got[b, r, col]) & 0xffffffff,
                                                     int(want[b, r, col]) & 0xffffffff))
    if not w['C'].outside_ok():
        bad.append(_outside_report(w['C'], 'C'))
    if c.bits == 'out':
        wb = pack_bits((t.ref[0].to(torch.float32).to(DTYPES[c.out]).float() > 0))
        gb = w['mbo'].read().cpu()
        if not torch.equal(gb, wb):
            r, g = (int(x) for x in (gb != wb)[0].nonzero()[0])
            bad.append('inside the bits_out window: %d words differ, first at (row %d, word %d)'
                       % (int((gb != wb).sum()), r, g))
        if not w['mbo'].outside_ok():
            bad.append(_outside_report(w['mbo'], 'bits_out'))
    for k, x in w.items():
        if k not in ('C', 'mbo') and not x.unchanged():
            bad.append('input buffer %s was written' % k)
    return '%s: %s' % (c.id, '; '.join(bad)) if bad else None


def _outside_report(x, name):
    keep = torch.ones(x.buf.numel(), dtype=torch.bool)
    keep[x.index] = False
    hit = (keep & (_ints(x.buf).cpu() != _canary(x.dtype))).nonzero().view(-1)
    e = int(hit[0]) - x.front
    where = 'before the first window' if e < 0 else 'row %d, col %d of the padded layout' % (
        (e % x.stride if x.stride else e) // x.ld, (e % x.stride if x.stride else e) % x.ld)
    return 'outside the %s window: %d canary elements overwritten, first at buffer element %d ' \
           '(%s)' % (name, hit.numel(), int(hit[0]), where)


def untouched(t):
    """The C buffer (and bits_out) is canary throughout: nothing was written (a refusal)."""
    xs = [t.w['C']] + ([t.w['mbo']] if 'mbo' in t.w else [])
    return all(bool((_ints(x.buf) == _canary(x.dtype)).all()) for x in xs)
