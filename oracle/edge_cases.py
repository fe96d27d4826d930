"""Edge-case catalogue of the inference launchers: every kernel ``pv_gemm_conv`` / ``pv_attention`` can dispatch to, and every other inference
launcher, at the smallest ragged shape that still selects it, audited element by element by ``oracle.plan_audit.Auditor``.

A case is a name, a function that records one or a few launches on a fresh ``EdgeRecorder`` with seeded inputs, and the per-call environment
switches that have to be set while it is recorded AND while it runs (the library reads them per call).  Shapes that depend on a dispatch threshold
are found by asking ``pv_gemm_conv_kernel_info`` / ``pv_attention_kernel_info`` (``first``), not by restating the rule.

Every tensor a launch addresses is a guarded view (``guarded_out`` / ``guarded_in``): it sits in the middle of a larger storage with at least
``TILE_ROWS`` = 256 rows x ld elements in front and behind (256 rows: the tallest tile of the library, so a whole stray tile stays inside the
storage the Auditor snapshots), and with a row gap (``ld = cols + 8``) wherever the launcher takes a leading dimension.  Output margins hold the
byte ``OUT_FILL``; input margins and row gaps hold NaN (0x7fffffff next to 32-bit integers, -1 next to 64-bit indices): an input's described extent is all a launch may depend
on, so anything read outside it that reaches a result makes the result non-finite, which the Auditor's finite check reports.  Reads inside an
arena cannot fault.  ``EdgeRecorder.empty`` guards the buffers the recorder allocates itself (workspaces, statistics, outputs), ``reguard`` the
inputs it derives at record time (folded weights, row sums).

The launchers of the newer loop features and of the pre-loop conditioning (the guided / stochastic / PAG steps, ``pv_freeu_rows``, the resize, the
fp32 pointwise ones, ``pv_rows_mean``, the casts, patchify and the two embeds) are not GEMMs: besides their smallest shapes a second group of cases
(name prefix ``product-``) runs single launches of them at the shapes the product gives them.  A case may promise that two of its launches are the
same kernel on the same inputs (``rec.same_bits``: pairs of outputs that must agree bit for bit - the launchers' documented substitutions).

A third group (prefix ``train-``) holds single launches of 25 launchers of the training tape - pointwise passes and their backwards, dropout, the layout
and exact-select launchers, the fixed-order reductions, the pieces of the identity loss, ``pv_layernorm_backward``, ``pv_wgrad_tn`` - at the smallest
shapes that reach their edges (a last 8-column chunk, a tail row, a second workgroup, every threshold of a dispatch from both sides, a one-row last
slab); no training plan is replayed.

With a CPU device the recorder is dry: it builds the same parameter blocks and tags (the ``*_kernel_info`` calls need no GPU) and never runs.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import zlib
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import torch

from . import abi_ref as A
from .plan_audit import Params

F16, F32, I32 = torch.float16, torch.float32, torch.int32
TILE_ROWS = 256
OUT_FILL = 0xA5
FLAT_CAP = 4096          # a buffer without rows (ld 0) is guarded by 256 x min(its length, FLAT_CAP) elements


def _isz(dt) -> int:
    return torch.empty((), dtype=dt).element_size()


def _arena(n_front: int, n_body: int, dtype, device, fill, arenas):
    total = n_front + n_body + n_front
    if fill == "out":
        a = torch.empty(total, dtype=dtype, device=device)
        a.view(torch.uint8).fill_(OUT_FILL)
    elif dtype.is_floating_point:
        a = torch.full((total,), float("nan"), dtype=dtype, device=device)
    elif dtype == torch.int64:
        # 64-bit integers are row indices (token ids, placeholder positions): -1 lands in the NaN margin in front of the table it indexes, which the
        # finite check reports; the largest value would send the read far outside every arena
        a = torch.full((total,), -1, dtype=dtype, device=device)
    else:
        a = torch.full((total,), torch.iinfo(dtype).max, dtype=dtype, device=device)
    if arenas is not None:
        arenas.append((a.data_ptr(), a.data_ptr() + total * _isz(dtype), a))
    return a


def guarded_out(rows: int, cols: int, dtype=F16, ld: Optional[int] = None, *, device="cpu", arenas=None) -> torch.Tensor:
    """A [rows, cols] view (row stride ``ld``, default ``cols``) with >= 256 x ld elements of ``OUT_FILL`` bytes in front and behind."""
    ld = cols if ld is None else ld
    assert ld >= cols, (cols, ld)
    m = TILE_ROWS * ld
    a = _arena(m, rows * ld, dtype, device, "out", arenas)
    return a[m:m + rows * ld].view(rows, ld)[:, :cols]


def guarded_in(t: torch.Tensor, ld: Optional[int] = None, *, device="cpu", arenas=None) -> torch.Tensor:
    """``t`` placed the same way, margins and row gaps NaN (integers: the largest value).  2-D: a row view with stride ``ld``; any other rank:
    contiguous, guarded by 256 x min(numel, FLAT_CAP) elements."""
    if t.dim() == 2:
        rows, cols = t.shape
        ld = cols if ld is None else ld
        m = TILE_ROWS * ld
        a = _arena(m, rows * ld, t.dtype, device, "in", arenas)
        v = a[m:m + rows * ld].view(rows, ld)[:, :cols]
    else:
        n = t.numel()
        m = TILE_ROWS * min(max(n, 1), FLAT_CAP)
        a = _arena(m, n, t.dtype, device, "in", arenas)
        v = a[m:m + n].view(t.shape)
    v.copy_(t)
    return v


def _recorder_base():
    from photoverse_amd.ops import Recorder
    return Recorder


def make_recorder(device):
    Recorder = _recorder_base()

    class EdgeRecorder(Recorder):
        """``ops.Recorder`` whose own allocations are guarded; dry (records, never runs) on a CPU device."""

        def __init__(self, dev):
            super().__init__(torch.device("cuda"))          # touches no device: loads the library and sets the lists
            self.device = torch.device(dev)
            self.dry = self.device.type != "cuda"
            self.arenas: list = []

        def empty(self, shape, dtype=F16):
            shape = (shape,) if isinstance(shape, int) else tuple(shape)
            n = math.prod(shape)
            row = min(max(n, 1), FLAT_CAP) if len(shape) == 1 else (shape[-1] if len(shape) == 2 else shape[-1] * shape[-2])
            m = TILE_ROWS * row
            a = _arena(m, n, dtype, self.device, "out", self.arenas)
            self.bytes_allocated += n * _isz(dtype)
            self.keep.append(a)
            return a[m:m + n].view(shape)

        def run(self, stream=None):
            if self.dry:
                raise RuntimeError("a dry EdgeRecorder holds host pointers: it describes launches, it cannot run them")
            return super().run(stream)

    return EdgeRecorder(device)


class Ctx:
    """What a case function gets: the recorder, a seeded generator and the guarded allocators."""

    def __init__(self, name: str, device):
        self.rec = make_recorder(device)
        self.dev = self.rec.device
        self.g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g) * scale

    def put(self, t: torch.Tensor, ld: Optional[int] = None) -> torch.Tensor:
        v = guarded_in(t, ld, device=self.dev, arenas=self.rec.arenas)
        self.rec.keep.append(v)
        return v

    def h(self, rows, cols, scale=1.0, gap=8):
        """fp16 rows of N(0, scale^2) with a row gap."""
        return self.put(self.randn(rows, cols, scale=scale).to(F16), cols + gap)

    def w(self, n, k):
        """a contiguous fp16 weight [n][k] of N(0, 1 / k)"""
        return self.put(self.randn(n, k, scale=k ** -0.5).to(F16))

    def f(self, *shape, scale=1.0, shift=0.0):
        return self.put(self.randn(*shape, scale=scale) + shift)

    def out(self, rows, cols, dtype=F16, gap=8):
        v = guarded_out(rows, cols, dtype, cols + gap, device=self.dev, arenas=self.rec.arenas)
        self.rec.keep.append(v)
        return v

    def out_flat(self, *shape, dtype=F32):
        return self.rec.empty(shape, dtype) if len(shape) == 1 else self.rec.empty((math.prod(shape),), dtype).view(shape)

    def colstats_for(self, x: torch.Tensor):
        """The column statistics a GEMM epilogue leaves for its contiguous fp16 output ``x`` ([ceil(M/64)][2][N] fp32 sums and sums of squares
        per 64-row block), computed here so that a consumer can be driven without its producer."""
        M, N = x.shape
        nb = (M + 63) // 64
        xf = torch.cat([x.float().cpu(), torch.zeros(nb * 64 - M, N)]).view(nb, 64, N)
        cs = self.put(torch.stack([xf.sum(1), (xf * xf).sum(1)], 1).contiguous())
        self.rec.colstats[(x.data_ptr(), M, N)] = cs
        return cs


# ------------------------------------------------------------------------------------------------------------------------------ the registry
@dataclass
class Case:
    name: str
    fn: Callable
    env: Dict[str, str] = field(default_factory=dict)
    expect: tuple = ()          # kernel symbols this case exists for: each must be among its tags


CASES: List[Case] = []


def add(name, fn, env=None, expect=()):
    CASES.append(Case(name, fn, dict(env or {}), tuple(expect)))


@contextlib.contextmanager
def environment(env: Dict[str, str], folds: bool = True):
    """The per-call switches of a case, and the recorder's two opt-in folds (``Recorder.GEMM_LN`` / ``GN_FOLD``, off by default) enabled."""
    Recorder = _recorder_base()
    old = {k: os.environ.get(k) for k in env}
    oldf = (Recorder.GEMM_LN, Recorder.GN_FOLD)
    os.environ.update(env)
    if folds:
        Recorder.GEMM_LN = Recorder.GN_FOLD = True
    try:
        yield
    finally:
        Recorder.GEMM_LN, Recorder.GN_FOLD = oldf
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(c: Case, device="cpu"):
    """Record the case on a fresh recorder (inside ``environment(c.env)``: the caller keeps it set while the launches run)."""
    ctx = Ctx(c.name, device)
    c.fn(ctx)
    reguard(ctx)
    return ctx.rec


def first(pred, candidates):
    for x in candidates:
        if pred(x):
            return x
    raise ValueError("no candidate selects the wanted kernel")


def gemm_symbol(**fields) -> str:
    return _recorder_base()._probe_gemm(**fields)


def attn_symbol(**fields) -> str:
    from photoverse_amd import _lib
    p = _lib.AttnParams()
    for k in ("q", "k", "v", "out"):
        setattr(p, k, 0x1000)
    for k, v in fields.items():
        setattr(p, k, v)
    try:
        return _lib.kernel_info(_lib.load().pv_attention_kernel_info, p)[0]
    except ValueError:
        return ""


# ------------------------------------------------------------------------------------------------------------------------------ guard checks
def _call_params(fn, args):
    name = fn.__name__
    if args and isinstance(args[0], type(C.byref(C.c_int()))):
        return name, Params(args[0]._obj, dict(zip(A.ARGS.get(name, ()), args[1:]))), args[0]._obj
    return name, Params(None, dict(zip(A.ARGS[name], args))), None


def _in_arena(arenas, addr, nbytes, margin):
    for lo, hi, _ in arenas:
        if lo <= addr < hi:
            return addr - lo >= margin and hi - (addr + nbytes) >= margin
    return False


def _extent(buf: A.Buf):
    isz = _isz(buf.dtype)
    ld = buf.ld if buf.ld else buf.cols
    ext = ((buf.rows - 1) * ld + buf.cols) * isz if buf.rows > 0 and buf.cols > 0 else 0
    margin = TILE_ROWS * (buf.ld if buf.ld else min(buf.cols, FLAT_CAP)) * isz
    return ext, margin


def unguarded(rec) -> List[str]:
    """Every pointer of every recorded call that is NOT a guarded view of its described extent (empty = the catalogue's placement rule holds)."""
    bad = []
    for i, (fn, args) in enumerate(rec.calls):
        name, p, _ = _call_params(fn, args)
        for k, buf in A.LAYOUT[name](p).items():
            addr = getattr(p, k)
            if not addr:
                continue
            buf = buf if buf is not None else A.Buf(F32, 1, 8, 0)          # extent known from device state only: its first row
            ext, margin = _extent(buf)
            if not _in_arena(rec.arenas, addr, ext, margin):
                bad.append(f"call {i} ({name}), field {k}")
    return bad


def host_views(rec, i: int):
    """(launcher, params, field -> [rows, cols] view) of call ``i`` of a DRY recorder, resolved through its arenas the way ``plan_audit.Auditor`` resolves a
    live one through the held storages: what ``abi_ref.REF`` is evaluated on without a GPU."""
    fn, args = rec.calls[i]
    name, p, _ = _call_params(fn, args)
    L = dict(A.LAYOUT[name](p))
    v = {}

    def resolve(k, buf):
        addr = getattr(p, k)
        if not addr:
            return
        lo, hi, a = next(e for e in rec.arenas if e[0] <= addr < e[1])
        assert a.dtype == buf.dtype, (name, k, a.dtype, buf.dtype)
        ld = buf.ld if buf.ld else buf.cols
        v[k] = a.as_strided((buf.rows, buf.cols), (ld, 1), (addr - lo) // _isz(buf.dtype))

    dep = A.DEPENDENT.get(name)
    if dep is not None and L.get(dep[0]) is not None:
        resolve(dep[0], L[dep[0]])
        if dep[0] in v:
            L[dep[1]] = dep[2](p, v[dep[0]])
    for k, buf in L.items():
        if k not in v and buf is not None:
            resolve(k, buf)
    if dep is not None and dep[3] and dep[1] in v:
        v[dep[1]] = v[dep[1]][:, A.step_index(v[dep[0]]) * dep[3]:][:, :dep[3]]
    return name, p, v


def reguard(ctx: Ctx):
    """Move the inputs the recorder derived at record time (LayerNorm-folded weights, bias folds, weight row sums) into guarded storage and
    point the parameter block at the copy."""
    rec = ctx.rec
    held = [t for t in rec.keep if isinstance(t, torch.Tensor)]
    for fn, args in rec.calls:
        name, p, struct = _call_params(fn, args)
        if struct is None:
            continue
        for k, buf in A.LAYOUT[name](p).items():
            addr = getattr(p, k)
            if not addr or buf is None or buf.role != "in":
                continue
            ext, margin = _extent(buf)
            if _in_arena(rec.arenas, addr, ext, margin):
                continue
            src = None
            for t in held:
                s = t.untyped_storage()
                if s.data_ptr() <= addr and addr + ext <= s.data_ptr() + s.nbytes() and t.dtype == buf.dtype:
                    ld = buf.ld if buf.ld else buf.cols
                    src = torch.empty(0, dtype=buf.dtype, device=t.device).set_(s, (addr - s.data_ptr()) // _isz(buf.dtype), (buf.rows, buf.cols), (ld, 1))
                    break
            if src is None:
                raise AssertionError(f"{name}: field {k} addresses no tensor the recorder holds")
            g = ctx.put(src.cpu().clone() if buf.rows > 1 else src.cpu().reshape(-1).clone(), None)
            setattr(struct, k, g.data_ptr())


# ============================================================================================================================== pv_gemm_conv
def _linear(ctx, M, N, K, *, bias=False, rowadd=None, rpi=None, residual=False, act=0, out_f32=False, geglu=False, splitk=0, colstats=False,
            dual=False, ln=False, a=None, wt=None, bias_t=None):
    """One Linear launch.  ``rowadd``: "shared" / "image" (rows_per_image ``rpi``); ``dual``: two strided sources of K / 2 channels each."""
    rec = ctx.rec
    n_out = N // 2 if geglu else N
    if a is None:
        a = (ctx.h(M, K // 2), ctx.h(M, K // 2)) if dual else (ctx.h(M, K), None)
    w = ctx.w(N, K) if wt is None else wt
    kw = {}
    if bias or bias_t is not None:
        kw["bias"] = ctx.f(N) if bias_t is None else bias_t
    if rowadd == "shared":
        kw["rowadd"] = ctx.f(n_out)
    elif rowadd == "image":
        imgs = (M + rpi - 1) // rpi
        ra = ctx.put(ctx.randn(imgs, n_out), n_out + 8)
        kw.update(rowadd=ra, rowadd_ld=ra.stride(0), rows_per_image=rpi)
    if residual:
        kw["residual"] = ctx.h(M, n_out)
    if ln:
        kw.update(ln_gamma=ctx.f(K, scale=0.2, shift=1.0), ln_beta=ctx.f(K, scale=0.2))
    out = ctx.out(M, n_out, F32 if out_f32 else F16, gap=0 if colstats else 8)       # column statistics need a contiguous output (ops.Recorder.gemm)
    rec.gemm(a[0], w, a1=a[1], out=out, act=act, out_f32=out_f32, geglu=geglu, splitk=splitk, colstats=colstats, **kw)
    return out


def _conv(ctx, batch, hin, win, c0, N, *, c1=0, stride=1, up=0, pad=1, splitk=0, colstats=False, bias=True, rowadd=False, residual=False, act=0,
          a_norm=None, a=None):
    rec = ctx.rec
    hl, wl = (hin * 2, win * 2) if up else (hin, win)
    if stride == 2:          # Conv2d(stride=2, padding=1), or F.pad(x, (0, 1, 0, 1)) + Conv2d(stride=2, padding=0) when pad == 0: torch's output sizes
        hout, wout = (hl + (2 if pad else 1) - 3) // 2 + 1, (wl + (2 if pad else 1) - 3) // 2 + 1
    else:
        hout, wout = hl, wl
    M = batch * hout * wout
    if a is None:
        a = (ctx.h(batch * hin * win, c0), ctx.h(batch * hin * win, c1) if c1 else None)
    w = ctx.w(N, 9 * (c0 + c1))
    kw = {}
    if bias:
        kw["bias"] = ctx.f(N)
    if rowadd:
        ra = ctx.put(ctx.randn(batch, N), N + 8)
        kw.update(rowadd=ra, rowadd_ld=ra.stride(0))
    if residual:
        kw["residual"] = ctx.h(M, N)
    if a_norm is not None:
        kw.update(a_norm=a_norm, a_norm_act=1)
    out = ctx.out(M, N, F16, gap=0 if colstats else 8)
    rec.gemm(a[0], w, a1=a[1], out=out, act=act, splitk=splitk, colstats=colstats,
             conv=dict(batch=batch, hin=hin, win=win, hout=hout, wout=wout, stride=stride, upsample=up, pad=pad), **kw)
    return out


def _lin_fields(M, N, K, **kw):
    f = dict(c0=K, lda0=K, N=N, ldc=N, M=M, taps=1, batch=1, hin=1, win=1, hout=M, wout=1, stride=1, pad=1)
    f.update(kw)
    return f


G64 = "gemm_conv_kernel<%d, false, false, false, false, 2>"
G128 = "gemm_conv_kernel<%d, false, false, false, false, 4>"

# 64-row kernels: M in {1, 65}, N in {160, 128}, one K-step and three; every epilogue feature and activation once per tile family
add("gemm64-n160-m1-k64-bias-silu-rowadd", lambda c: _linear(c, 1, 160, 64, bias=True, act=1, rowadd="shared"), expect=(G64 % 5,))
add("gemm64-n160-m65-k192-rowadd-per-image-res-qgelu", lambda c: _linear(c, 65, 160, 192, rowadd="image", rpi=40, residual=True, act=2), expect=(G64 % 5,))
add("gemm64-n160-m65-k128-dual-f32", lambda c: _linear(c, 65, 160, 128, dual=True, out_f32=True, bias=True), expect=(G64 % 5,))
add("gemm64-n128-m1-k192-f32-leaky-bias", lambda c: _linear(c, 1, 128, 192, out_f32=True, act=3, bias=True), expect=(G64 % 4,))
add("gemm64-n128-m65-k64-res-rowadd", lambda c: _linear(c, 65, 128, 64, residual=True, rowadd="shared", act=1), expect=(G64 % 4,))
add("gemm64-n128-m65-k128-dual-rowadd-per-image-qgelu", lambda c: _linear(c, 65, 128, 128, dual=True, rowadd="image", rpi=40, act=2, bias=True), expect=(G64 % 4,))


def _m_for_128_row_kernel(N, nf):
    """Smallest M = 128 t + 65 whose launch count puts a plain Linear on the 128-row kernel (asked from the library)."""
    return first(lambda M: gemm_symbol(**_lin_fields(M, N, 64)) == G128 % nf, (128 * t + 65 for t in range(0, 4096)))


add("gemm128-n1280-by-count-bias-silu-rowadd-per-image", lambda c: _linear(c, _m_for_128_row_kernel(1280, 5), 1280, 64, bias=True, act=1, rowadd="image", rpi=100),
    expect=(G128 % 5,))
add("gemm128-n1024-by-count-res-leaky-f32", lambda c: _linear(c, _m_for_128_row_kernel(1024, 4), 1024, 64, residual=True, act=3, out_f32=True, rowadd="shared"),
    expect=(G128 % 4,))
for _sk, _n, _nf in ((2, 160, 5), (3, 128, 4), (3, 160, 5), (2, 128, 4)):
    add(f"gemm128-splitk{_sk}-n{_n}-m130-k192-colstats", lambda c, sk=_sk, n=_n: _linear(c, 130, n, 192, splitk=sk, colstats=True, bias=True, act=1, residual=sk == 3),
        expect=(G128 % _nf,))
for _n, _nf in ((160, 5), (128, 4)):
    add(f"gemm-colstats-n{_n}-m130", lambda c, n=_n: _linear(c, 130, n, 64, colstats=True, bias=True, act=1, rowadd="image", rpi=50),
        expect=("gemm_conv_kernel<%d, false, false, true, false, 4>" % _nf,))
add("gemm-geglu-n256-m130", lambda c: _linear(c, 130, 256, 64, geglu=True, bias=True), expect=("gemm_conv_kernel<4, false, true, false, false, 4>",))
GEGLU_LOOP = "gemm_conv_kernel<4, false, true, false, true, 4>"


def _geglu_loop(c):
    M = first(lambda M: gemm_symbol(**_lin_fields(M, 256, 64, geglu=1, ldc=128)) == GEGLU_LOOP, (128 * t + 1 for t in range(0, 4096)))
    _linear(c, M, 256, 64, geglu=True, bias=True)


add("gemm-geglu-tile-loop-smallest-m", _geglu_loop, expect=(GEGLU_LOOP,))

# 3x3 convs: batch 2, a 5 x 7 image, 64 channels
C9 = "gemm_conv_kernel<%d, true, false, %s, false, 4>"
add("conv-s1-n160-rowadd-silu", lambda c: _conv(c, 2, 5, 7, 64, 160, rowadd=True, act=1), expect=(C9 % (5, "false"),))
add("conv-s1-n128-res", lambda c: _conv(c, 2, 5, 7, 64, 128, residual=True), expect=(C9 % (4, "false"),))
add("conv-s2-pad1-n128", lambda c: _conv(c, 2, 5, 7, 64, 128, stride=2), expect=(C9 % (4, "false"),))
add("conv-s2-pad0-n160", lambda c: _conv(c, 2, 5, 7, 64, 160, stride=2, pad=0), expect=(C9 % (5, "false"),))
add("conv-up2-n128-res-silu", lambda c: _conv(c, 2, 5, 7, 64, 128, up=1, residual=True, act=1), expect=(C9 % (4, "false"),))
add("conv-dual-n160", lambda c: _conv(c, 2, 5, 7, 64, 160, c1=64, rowadd=True), expect=(C9 % (5, "false"),))
add("conv-dual-s2-pad1-n128", lambda c: _conv(c, 2, 5, 7, 64, 128, c1=64, stride=2), expect=(C9 % (4, "false"),))
for _sk, _n, _nf in ((2, 160, 5), (3, 128, 4), (5, 160, 5), (8, 128, 4), (5, 128, 4), (8, 160, 5)):
    add(f"conv-splitk{_sk}-n{_n}", lambda c, sk=_sk, n=_n: _conv(c, 2, 5, 7, 64, n, splitk=sk, colstats=sk in (2, 8), act=1), expect=(C9 % (_nf, "false"),))
for _n, _nf in ((160, 5), (128, 4)):
    add(f"conv-colstats-n{_n}", lambda c, n=_n: _conv(c, 2, 5, 7, 64, n, colstats=True, rowadd=True, act=1), expect=(C9 % (_nf, "true"),))

# the 256-row tile (big_min = 1 puts a one-tile launch on it)
BIG = "big_tile_kernel<%s, %s, 8, %d, %s>"


def _big(fn):
    def run(c):
        c.rec.big_min = 1
        fn(c)
    return run


for _cs in (False, True):
    _t = "true" if _cs else "false"
    add(f"big-linear-m257-k640-n320{'-colstats' if _cs else ''}", _big(lambda c, cs=_cs: _linear(c, 257, 320, 640, bias=True, act=1, residual=True, colstats=cs, rowadd="image", rpi=100)),
        expect=(BIG % (_t, "false", 1, "false"),))
    add(f"big-conv-gather-10x10{'-colstats' if _cs else ''}", _big(lambda c, cs=_cs: _conv(c, 1, 10, 10, 64, 320, colstats=cs, rowadd=True, act=1, residual=True)),
        expect=(BIG % (_t, "false", 0, "false"),))
    add(f"big-conv-upsample-5x5{'-colstats' if _cs else ''}", _big(lambda c, cs=_cs: _conv(c, 1, 5, 5, 64, 320, up=1, colstats=cs)), expect=(BIG % (_t, "true", 0, "false"),))
    add(f"big-conv-patch64-4x64{'-colstats' if _cs else ''}", _big(lambda c, cs=_cs: _conv(c, 1, 4, 64, 64, 320, colstats=cs, rowadd=True, act=1, residual=True)),
        expect=(BIG % (_t, "false", 3, "false"),))
    add(f"big-conv-patch32-8x32{'-colstats' if _cs else ''}", _big(lambda c, cs=_cs: _conv(c, 1, 8, 32, 64, 320, colstats=cs, act=1)), env={"PV_CONV_PATCH": "1"},
        expect=(BIG % (_t, "false", 4, "false"),))
add("big-geglu-m257-k640-n256", _big(lambda c: _linear(c, 257, 256, 640, geglu=True, bias=True)), expect=(BIG % ("false", "false", 2, "false"),))
add("big-linear-layernorm-fold", _big(lambda c: _linear(c, 257, 320, 640, ln=True, bias=True, act=1)), expect=(BIG % ("false", "false", 1, "true"),))
add("big-geglu-layernorm-fold", _big(lambda c: _linear(c, 257, 256, 640, ln=True, geglu=True, bias=True)), expect=(BIG % ("false", "false", 2, "true"),))
add("big-conv-splitk2-cin128", _big(lambda c: _conv(c, 1, 10, 10, 128, 320, splitk=2, colstats=True, act=1)), expect=(BIG % ("false", "false", 0, "false"),))
add("big-conv-upsample-splitk2-cin128", _big(lambda c: _conv(c, 1, 5, 5, 128, 320, up=1, splitk=2)), expect=(BIG % ("false", "true", 0, "false"),))
add("big-conv-patch64-batch2", _big(lambda c: _conv(c, 2, 4, 64, 64, 320, act=1)), expect=(BIG % ("false", "false", 3, "false"),))
add("big-conv-patch64-dual", _big(lambda c: _conv(c, 1, 4, 64, 64, 320, c1=64, rowadd=True)), expect=(BIG % ("false", "false", 3, "false"),))
add("big-conv-patch32-batch2-dual", _big(lambda c: _conv(c, 2, 8, 32, 64, 320, c1=64)), env={"PV_CONV_PATCH": "1"}, expect=(BIG % ("false", "false", 4, "false"),))


def _gn_fold_conv(c, batch, h, w, c0, c1, colstats):
    """pv_groupnorm_scale_shift on the raw tensors' column statistics, then the conv that normalises its LDS-resident patch with the table."""
    c.rec.big_min = 1
    x0 = c.put(c.randn(batch * h * w, c0, scale=1.5).add_(0.5).to(F16))
    x1 = c.put(c.randn(batch * h * w, c1).to(F16)) if c1 else None
    c.colstats_for(x0)
    if c1:
        c.colstats_for(x1)
    tab = c.rec.groupnorm_table(x0, c.f(c0 + c1, scale=0.3, shift=1.0), c.f(c0 + c1, scale=0.2), batch=batch, hw=h * w, x1=x1)
    assert tab is not None
    _conv(c, batch, h, w, c0, 320, c1=c1, colstats=colstats, a_norm=tab, a=(x0, x1), act=1)


for _cs in (False, True):
    _t = "true" if _cs else "false"
    add(f"big-conv-groupnorm-fold-patch64{'-colstats' if _cs else ''}", lambda c, cs=_cs: _gn_fold_conv(c, 1, 4, 64, 64, 0, cs), expect=(BIG % (_t, "false", 5, "false"),))
    add(f"big-conv-groupnorm-fold-patch32{'-colstats' if _cs else ''}", lambda c, cs=_cs: _gn_fold_conv(c, 1, 8, 32, 64, 0, cs), env={"PV_CONV_PATCH": "1"},
        expect=(BIG % (_t, "false", 6, "false"),))
add("big-conv-groupnorm-fold-patch64-batch2-dual", lambda c: _gn_fold_conv(c, 2, 4, 64, 64, 64, False), expect=(BIG % ("false", "false", 5, "false"),))


# ============================================================================================================================== pv_attention
def _attention(ctx, batch, heads, nq, nk, d, *, causal=False, lse=False, sliced=True, hot_key=False, zero=False):
    """q / k / v: column slices of one [rows][3 C + 8] buffer when nq == nk (the fused QKV GEMM's output), separate strided buffers otherwise."""
    Cw = heads * d
    if sliced and nq == nk:
        qkv = ctx.randn(batch * nq, 3 * Cw)
        if zero:
            qkv.zero_()
        buf = ctx.put(qkv.to(F16), 3 * Cw + 8)
        q, k, v = buf[:, :Cw], buf[:, Cw:2 * Cw], buf[:, 2 * Cw:]
    else:
        qt, kt = ctx.randn(batch * nq, Cw), ctx.randn(batch * nk, Cw)
        if hot_key:
            # the queries share a unit offset and the last key of every image (in the last, partial key block) points along it with length 12:
            # its score is 12 (+- 12 / sqrt d) against the other keys' ~1.4 sigma
            qt += 1.0
            for b in range(batch):
                kt[b * nk + nk - 1] = 12.0 / math.sqrt(d)
        q, k, v = ctx.put(qt.to(F16), Cw + 8), ctx.put(kt.to(F16), Cw + 8), ctx.h(batch * nk, Cw, gap=16)
    out = ctx.out(batch * nq, Cw)
    l = ctx.out_flat(batch, heads, nq) if lse else None
    ctx.rec.attention(q, k, v, batch=batch, heads=heads, nq=nq, nk=nk, d=d, causal=causal, out=out, lse=l)


def _attn_set(d):
    def run(c):
        for nq, nk, kw in ((1, 65, dict(lse=True)), (65, 1, {}), (130, 63, {}), (63, 64, dict(lse=True)), (65, 65, dict(causal=True, lse=True)), (77, 77, dict(causal=True)),
                           (65, 65, {})):
            _attention(c, 2, 2, nq, nk, d, **kw)
    return run


for _d in (64, 80, 160):
    add(f"attention-d{_d}-ragged", _attn_set(_d), expect=(f"attn_kernel<{_d}, 2, false>",))
add("attention-d40-ragged", _attn_set(40), expect=("attn_kernel<40, 2, true>",))
A40_4 = "attn_kernel<40, 4, true>"


def _bh_for_four_fragments(**kw):
    return first(lambda bh: attn_symbol(batch=bh // 8, heads=8, nq=257, nk=257, d=40, ldq=968, ldk=968, ldv=968, ldo=328, **kw) == A40_4, range(8, 8192, 8))


add("attention-d40-four-fragments-causal-nq257", lambda c: _attention(c, _bh_for_four_fragments(causal=1) // 8, 8, 257, 257, 40, causal=True, lse=True), expect=(A40_4,))
add("attention-d40-four-fragments-nq257", lambda c: _attention(c, _bh_for_four_fragments() // 8, 8, 257, 257, 40), env={"PV_ATTN8": "-1"}, expect=(A40_4,))
add("attention-d40-8wave-n600", lambda c: _attention(c, 1, 2, 600, 600, 40, lse=True), env={"PV_ATTN8_MIN": "1"}, expect=("attn8_kernel<497>",))
add("attention-d40-8wave-nq600-nk77", lambda c: _attention(c, 1, 2, 600, 77, 40), env={"PV_ATTN8_MIN": "1"}, expect=("attn8_kernel<497>",))
for _d in (40, 80):
    add(f"attention-d{_d}-hot-key-in-the-partial-block", lambda c, d=_d: _attention(c, 2, 2, 130, 65, d, hot_key=True, lse=True))
add("attention-d64-all-zero", lambda c: _attention(c, 1, 2, 65, 65, 64, zero=True, lse=True))


# ============================================================================================================================== cross attention
def _kv(ctx, batch, nt, nip, Cw):
    return ctx.h(batch * nt, Cw), ctx.h(batch * nt, Cw, gap=16), (ctx.h(batch * nip, Cw) if nip else None), (ctx.h(batch * nip, Cw, gap=24) if nip else None)


def _xattn(ctx, batch, heads, nq, nt, nip, d, *, vnorm=False, fusion=None):
    Cw = heads * d
    q = ctx.h(batch * nq, Cw)
    kt, vt, kip, vip = _kv(ctx, batch, nt, nip, Cw)
    vn = ctx.out_flat(batch, heads, nip) if vnorm else None
    fu = ctx.put(torch.tensor(fusion, dtype=F32)) if fusion else None
    ctx.rec.cross_attention(q, kt, vt, kip, vip, batch=batch, heads=heads, nq=nq, nt=nt, nip=nip, d=d, vnorm=vn, fusion=fu, out=ctx.out(batch * nq, Cw),
                            w_text=1.0 if fusion is None else 7.0, w_ip=1.0 if fusion is None else 7.0)      # a device pair overrides the host weights


for _i, _d in enumerate((40, 80, 160)):
    for _j, (_nt, _nip) in enumerate(((1, 16), (77, 1), (80, 2))):
        _fu = (None, (2.0, 0.0), (0.0, 2.0))[(_i + _j) % 3]
        if _fu is not None and (_nt, _nip)[0 if _fu[0] else 1] == 1:      # keep the weight on the many-key branch: a one-key softmax is a copy
            _fu = _fu[::-1]
        add(f"xattn-d{_d}-nt{_nt}-nip{_nip}", lambda c, d=_d, nt=_nt, nip=_nip, vn=(_i + _j) % 2 == 0, fu=_fu: _xattn(c, 2, 2, 130, nt, nip, d, vnorm=vn, fusion=fu))
    # xattn_kernel<D, true>: >= 2048 query tiles of 128 rows in the launch (pv_attn.hip keeps ~1024 workgroups): nq = 130 is two tiles per (image, head)
    add(f"xattn-d{_d}-multi-tile", lambda c, d=_d: _xattn(c, 128, 8, 130, 77, 2, d, vnorm=True))


def _lnq(ctx, batch, heads, d, nq, nt, nip, *, ln, vnorm=False, fusion=None):
    Cw = heads * d
    hs = ctx.put((ctx.randn(batch * nq, Cw) * 1.5 + 0.5).to(F16), Cw + 8)
    kt, vt, kip, vip = _kv(ctx, batch, nt, nip, Cw)
    kw = dict(ln_gamma=ctx.f(Cw, scale=0.2, shift=1.0), ln_beta=ctx.f(Cw, scale=0.2)) if ln else {}
    vn = ctx.out_flat(batch, heads, nip) if vnorm else None
    fu = ctx.put(torch.tensor(fusion, dtype=F32)) if fusion else None
    ctx.rec.cross_attention_lnq(hs, ctx.w(Cw, Cw), kt, vt, kip, vip, batch=batch, heads=heads, nq=nq, nt=nt, nip=nip, d=d, vnorm=vn, fusion=fu,
                                out=ctx.out(batch * nq, Cw), **kw)


add("lnq-d160-nip0-nt80-ln", lambda c: _lnq(c, 1, 8, 160, 200, 80, 0, ln=True))
add("lnq-d160-nip16-nt1", lambda c: _lnq(c, 2, 2, 160, 200, 1, 16, ln=False, vnorm=True))
add("lnq-d160-nip1-nt80-ln-fusion", lambda c: _lnq(c, 1, 2, 160, 200, 80, 1, ln=True, fusion=(2.0, 0.0)))
add("lnq-d80-nip1-nt80-ln", lambda c: _lnq(c, 1, 8, 80, 200, 80, 1, ln=True, vnorm=True))
add("lnq-d80-nip16-nt1-ln-fusion", lambda c: _lnq(c, 2, 4, 80, 200, 1, 16, ln=True, fusion=(0.0, 2.0)))
add("lnq-d80-nip0-nt80", lambda c: _lnq(c, 1, 4, 80, 200, 80, 0, ln=False))


def _fused(ctx, Cw, batch, nt, nip, *, ln, rows=0, fusion=None, vnorm=True):
    heads, d, nq = 8, Cw // 8, 128
    rec = ctx.rec
    kt, vt, kip, vip = _kv(ctx, batch, nt, nip, Cw)
    vn = ctx.out_flat(batch, heads, nip) if vnorm else None
    kimg, vimg = rec.xattn_pack_kv(kt, vt, kip, vip, batch=batch, heads=heads, d=d, nt=nt, nip=nip, vnorm=vn)
    hs = ctx.put((ctx.randn(batch * nq, Cw) * 1.5 + 0.5).to(F16), Cw + 8)
    kw = dict(ln_gamma=ctx.f(Cw, scale=0.2, shift=1.0), ln_beta=ctx.f(Cw, scale=0.2)) if ln else {}
    fu = ctx.put(torch.tensor(fusion, dtype=F32)) if fusion else None
    # wo: the packed matrix itself is drawn (the reference unpacks it with pv_xattn_fused_wo_slot)
    _, p = rec.cross_attention_fused(hs, ctx.w(Cw, Cw), ctx.w(Cw, Cw), ctx.f(Cw), kimg, vimg, batch=batch, nq=nq, heads=heads, d=d, nt=nt, nip=nip, fusion=fu,
                                     out=ctx.out(batch * nq, Cw), **kw)
    p.rows_per_workgroup = rows


add("fused-c320-b1-nt65-nip1-ln", lambda c: _fused(c, 320, 1, 65, 1, ln=True))
add("fused-c320-b3-nt77-nip2", lambda c: _fused(c, 320, 3, 77, 2, ln=False, fusion=(2.0, 0.0)))
add("fused-c320-b1-nt80-nip16-ln", lambda c: _fused(c, 320, 1, 80, 16, ln=True, fusion=(1.0, 1.0), vnorm=False))
add("fused-c640-b1-nt65-nip16-ln-rows64", lambda c: _fused(c, 640, 1, 65, 16, ln=True, rows=64))
add("fused-c640-b3-nt80-nip1-rows128", lambda c: _fused(c, 640, 3, 80, 1, ln=False, rows=128, fusion=(0.0, 2.0)))
add("fused-c640-b1-nt77-nip2-ln-rows128", lambda c: _fused(c, 640, 1, 77, 2, ln=True, rows=128, vnorm=False))
add("fused-c640-b3-nt77-nip1-ln", lambda c: _fused(c, 640, 3, 77, 1, ln=True))


# ============================================================================================================================== pv_row_gemm
def _row_gemm(ctx, M, N, *, ln, geglu, bias, x_norm_rpi=0, const_row=False):
    x = ctx.randn(M, 320) * 1.5 + 0.5
    if const_row:
        x[M // 2] = 0.3                                      # zero variance (0.3 is no dyadic number: its fp32 sums round): the normalised row is 0, the result the folded bias
    kw = {}
    if ln:
        kw.update(ln_gamma=ctx.f(320, scale=0.2, shift=1.0), ln_beta=ctx.f(320, scale=0.2))
    if x_norm_rpi:
        tab = torch.stack([1.0 + 0.2 * ctx.randn(M // x_norm_rpi, 320), 0.3 * ctx.randn(M // x_norm_rpi, 320)], 1)
        kw.update(x_norm=ctx.put(tab.contiguous()), rows_per_image=x_norm_rpi)
    ctx.rec.row_gemm(ctx.put(x.to(F16), 328), ctx.w(N, 320), bias=ctx.f(N) if bias else None, geglu=geglu, out=ctx.out(M, N // 2 if geglu else N), **kw)


add("rowgemm-m1-ln-bias", lambda c: _row_gemm(c, 1, 320, ln=True, geglu=False, bias=True))
add("rowgemm-m257-ln-geglu", lambda c: _row_gemm(c, 257, 640, ln=True, geglu=True, bias=False))
add("rowgemm-m257-plain", lambda c: _row_gemm(c, 257, 960, ln=False, geglu=False, bias=False))
add("rowgemm-m1-geglu-bias", lambda c: _row_gemm(c, 1, 640, ln=False, geglu=True, bias=True))
add("rowgemm-m257-ln-geglu-bias", lambda c: _row_gemm(c, 257, 640, ln=True, geglu=True, bias=True))
add("rowgemm-m256-groupnorm-table-two-images", lambda c: _row_gemm(c, 256, 320, ln=False, geglu=False, bias=True, x_norm_rpi=128))
add("rowgemm-m257-ln-constant-row", lambda c: _row_gemm(c, 257, 320, ln=True, geglu=False, bias=True, const_row=True))


# ============================================================================================================================== norms
def _layernorm(ctx, rows, cols, *, act=0, const_row=False, zero=False):
    x = ctx.randn(rows, cols) * 1.5 + 0.5
    if const_row:
        x[rows // 2] = -2.3                                  # zero variance, sums that round: y = beta
    if zero:
        x.zero_()
    ctx.rec.layernorm(ctx.put(x.to(F16), cols + 8), ctx.f(cols, scale=0.2, shift=1.0), ctx.f(cols, scale=0.2), act=act, out=ctx.out(rows, cols, gap=16))


for _cols in (8, 320, 4096):
    for _rows in (1, 77):
        add(f"layernorm-{_rows}x{_cols}", lambda c, r=_rows, k=_cols: _layernorm(c, r, k, act=3 if k == 8 else 0))
add("layernorm-constant-row-77x320", lambda c: _layernorm(c, 77, 320, const_row=True))
add("layernorm-constant-row-77x640", lambda c: _layernorm(c, 77, 640, const_row=True))
add("layernorm-all-zero-5x320", lambda c: _layernorm(c, 5, 320, zero=True))


def _groupnorm(ctx, batch, hw, c0, c1=0, *, act=0, from_colstats=False, const_group=False):
    x0 = ctx.randn(batch * hw, c0) * 1.5 + 0.5
    if const_group:
        x0[:hw, : c0 // 32] = 1.3                            # group 0 of image 0: zero variance, sums that round: y = beta
    gap = 0 if from_colstats else 8
    x0 = ctx.put(x0.to(F16), c0 + gap)
    x1 = ctx.put(ctx.randn(batch * hw, c1).to(F16), c1 + gap) if c1 else None
    if from_colstats:
        ctx.colstats_for(x0)
        if c1:
            ctx.colstats_for(x1)
    ctx.rec.groupnorm(x0, ctx.f(c0 + c1, scale=0.2, shift=1.0), ctx.f(c0 + c1, scale=0.2), batch=batch, hw=hw, x1=x1, act=act)


add("groupnorm-hw1-c64", lambda c: _groupnorm(c, 3, 1, 64))
add("groupnorm-hw25-c2560-silu", lambda c: _groupnorm(c, 3, 25, 2560, act=1))
add("groupnorm-hw25-c64-dual", lambda c: _groupnorm(c, 3, 25, 32, 32))
add("groupnorm-hw64-c2560-dual", lambda c: _groupnorm(c, 3, 64, 1280, 1280, act=1))
add("groupnorm-hw64-c64-from-colstats", lambda c: _groupnorm(c, 3, 64, 64, from_colstats=True))
add("groupnorm-hw64-c2560-dual-from-colstats", lambda c: _groupnorm(c, 3, 64, 1280, 1280, from_colstats=True, act=1))
add("groupnorm-hw25-c64-constant-group", lambda c: _groupnorm(c, 3, 25, 64, const_group=True))
add("groupnorm-hw64-c64-constant-group-from-colstats", lambda c: _groupnorm(c, 3, 64, 64, const_group=True, from_colstats=True))


# ============================================================================================================================== small launchers
def _conv_out(c, cout):
    c.rec.conv_out(c.put(c.randn(2 * 5 * 7, 64).to(F16)), c.w(cout, 9 * 64), c.f(cout), batch=2, cin=64, h=5, wd=7, cout=cout, out=c.out_flat(2, cout, 5, 7))


add("conv-out-5x7-cout4", lambda c: _conv_out(c, 4))
add("conv-out-5x7-cout3", lambda c: _conv_out(c, 3))


def _state(c, idx, rows):
    return c.put(torch.tensor([idx, rows], dtype=I32))


def _timestep(c):
    c.rec.timestep_embedding(c.put(torch.tensor([999.0, 500.5, 1.0])), None, 3, 320)
    table = [981.0, 961.0, 941.0, 921.0, 901.0, 881.0, 861.0, 1.0]
    c.rec.timestep_embedding(c.put(torch.tensor(table)), _state(c, 3, 8), 1, 1280)
    c.rec.timestep_embedding(c.put(torch.tensor(table)), _state(c, 19, 8), 3, 6)       # a step past the table reads its last row


add("timestep-embedding-rows3", _timestep)


def _cfg(c, masked):
    B, ch, h, w = 2, 4, (6 if masked else 5), (6 if masked else 7)          # the masked form needs hw % 4 == 0
    steps = 5
    coef = c.put(torch.cat([c.randn(steps, 7, scale=0.5) + torch.tensor([1.0, -0.5, 0.8, 0.6, -0.3, 0.9, 0.4]), torch.zeros(steps, 1)], 1).contiguous())
    for idx in (0, 1, steps - 1):
        t = [c.f(B, ch, h, w) for _ in range(4)]
        if masked:
            m = torch.rand(B, 1, h, w, generator=c.g)
            m[0, 0, :2] = 1.0
            m[0, 0, 2:4] = 0.0
            c.rec.cfg_dpm_step_masked(*t, coef, _state(c, idx, steps), 7.5, c.put(m), c.f(B, ch, h, w), c.f(B, ch, h, w))
        else:
            c.rec.cfg_dpm_step(*t, coef, _state(c, idx, steps), 7.5)


add("cfg-dpm-step-5x7-steps-0-1-last", lambda c: _cfg(c, False))
add("cfg-dpm-step-masked-6x6-steps-0-1-last", lambda c: _cfg(c, True))
add("pointwise-nchw-5x7", lambda c: c.rec.pointwise_nchw(c.f(2, 4, 35), c.f(4, 4), c.f(4), batch=2, cin=4, cout=4, hw=35))
add("posterior-sample-5x7", lambda c: c.rec.posterior_sample(c.f(2, 8, 5, 7, scale=3.0), c.f(2, 4, 5, 7), out=c.out_flat(2 * 4 * 5 * 7).view(2, 4, 5, 7)))
add("im2col-5x7-kpad64", lambda c: c.rec.im2col3x3(c.f(2, 4, 5, 7), batch=2, cin=4, h=5, wd=7, kpad=64))
# pv_softmax_rows takes cols % 8 == 0 only (header): the ragged extents are the row counts 77 / 257 and the first valid widths above them
add("softmax-rows-77x80", lambda c: c.rec.softmax_rows(c.h(77, 80, scale=3.0), scale=0.3))
add("softmax-rows-257x264", lambda c: c.rec.softmax_rows(c.h(257, 264, scale=3.0), scale=0.05))


# ============================================================================================================================== value edges
def _cancelling(c):
    """[x | x] . [w | -w]^T: every product has its negative in the sum, the exact result is the bias."""
    x = c.randn(130, 64).to(F16)
    w = c.randn(160, 64, scale=0.125).to(F16)
    _linear(c, 130, 160, 128, a=(c.put(x, 72), c.put(x.clone(), 80)), wt=c.put(torch.cat([w, -w], 1).contiguous()), bias=True)


def _zero_gemm(c):
    _linear(c, 130, 160, 64, a=(c.put(torch.zeros(130, 64, dtype=F16), 72), None), bias=True, act=1)
    _conv(c, 2, 5, 7, 64, 128, a=(c.put(torch.zeros(70, 64, dtype=F16), 72), None), bias=False)


add("gemm-cancelling-operands", _cancelling)
add("gemm-all-zero-input", _zero_gemm)


# ============================================================================================================================== guided / stochastic / PAG steps
STEP_ROWS = 5
#: (C, h, w) with nv = C h w / 4 float4s per sample: one live lane of the one wave; 36; a second wave with one live lane; 1025 = one thread of the
#: 1024-thread workgroup takes a second trip of the strided loop.  hw % 4 == 0 is the launchers' rule (the mask is read as float4)
STEP_SHAPES = {1: (1, 2, 2), 36: (4, 6, 6), 65: (5, 4, 13), 1025: (5, 20, 41)}
#: rng words with the high bit set in every word; sample offset 0xFFFFFFFE: sample 2 wraps to counter word 0
STEP_RNG = (0x9E3779B9, 0xDEADBEEF, 0xFFFFFFFE, 0x80000003)
G_TEXT, G_IMAGE, G_PAG, RESCALE = 7.5, 3.0, 2.0, 0.7


def _i32(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=I32)


def _step_coef(c):
    """5 rows {ca, cb, cx, c0, c1, q0, q1, cn} around a mid-schedule row; the last row is the SDE table's last: cx = 0, c0 = 1, c1 = 0, cn = 0."""
    tab = torch.tensor([1.0, -0.5, 0.8, 0.6, -0.3, 0.9, 0.4, 0.7]) + 0.1 * c.randn(STEP_ROWS, 8)
    tab[-1, [2, 3, 4, 7]] = torch.tensor([0.0, 1.0, 0.0, 0.0])
    return c.put(tab.contiguous())


def _step_eps(c, shape, k):
    """One prediction (B = 3): sample 0 ordinary, sample 1 all zero, sample 2 constant - a dyadic value per prediction, so that every fp32 sum and the
    mean of the sample are exact and its deviations are exactly 0 beside a mean that is not (std = 0 next to an ordinary sample)."""
    t = c.randn(*shape)
    t[1] = 0.0
    t[2] = (0.5, 0.25, -0.75, 1.0)[k]
    return t


def _step_mask(c, B, h, w):
    m = torch.rand(B, 1, h, w, generator=c.g)
    flat = m.view(B, -1)
    flat[:, 0::4] = 1.0
    flat[:, 1::4] = 0.0                                   # ones, zeros and fractions in every float4
    return c.put(m.view(B, h * w)).view(B, 1, h, w)          # rows of hw elements: the margins are 256 whole rows, as the layout describes the mask


def _steps(kind, nv, *, pag_rng=False):
    """Every form of one step launcher at one size: two-forward + rescale, three-forward, three-forward + rescale, each without and with a mixed mask,
    each at the step indices 0, 1 and last."""
    ch, h, w = STEP_SHAPES[nv]
    shape = (3, ch, h, w)

    def run(c):
        rec = c.rec
        coef = _step_coef(c)
        eu, em, ec, ep = (c.put(_step_eps(c, shape, k)) for k in range(4))
        mask, known, noise = _step_mask(c, 3, h, w), c.f(*shape), c.f(*shape)
        rng = c.put(_i32(STEP_RNG)) if kind == "stochastic" or pag_rng else None
        for img, rs in ((None, RESCALE), (em, 0.0), (em, RESCALE)):
            for blend in ({}, dict(mask=mask, known=known, noise=noise)):
                for idx in (0, 1, STEP_ROWS - 1):
                    x, xp, st = c.f(*shape), c.f(*shape), _state(c, idx, STEP_ROWS)
                    if kind == "guided":
                        rec.cfg_dpm_step_guided(eu, img, ec, x, xp, coef, st, G_TEXT, G_IMAGE, rs, **blend)
                    elif kind == "stochastic":
                        rec.cfg_dpm_step_stochastic(eu, img, ec, x, xp, coef, st, rng, G_TEXT, G_IMAGE, rs, **blend)
                    else:
                        rec.cfg_dpm_step_pag(eu, img, ec, ep, x, xp, coef, st, G_TEXT, G_IMAGE, G_PAG, rs, rng=rng, **blend)
    return run


for _nv in STEP_SHAPES:
    add(f"step-guided-nv{_nv}", _steps("guided", _nv))
    add(f"step-stochastic-nv{_nv}", _steps("stochastic", _nv))
    add(f"step-pag-nv{_nv}", _steps("pag", _nv))
    add(f"step-pag-rng-nv{_nv}", _steps("pag", _nv, pag_rng=True))


def _step_substitutions(c):
    """The launcher's own substitutions, on inputs that are all NaN where they must not be read: eps_perturbed with g_pag = 0 is the guided launch (its
    outputs must have that launch's bits: ``same_bits``), eps_image at g_image == g_text the two-forward one."""
    ch, h, w = STEP_SHAPES[36]
    shape = (3, ch, h, w)
    rec = c.rec
    coef, st = _step_coef(c), _state(c, 1, STEP_ROWS)
    eu, em, ec = (c.put(_step_eps(c, shape, k)) for k in range(3))
    unread = c.put(torch.full(shape, float("nan")))
    x, xp = c.randn(*shape), c.randn(*shape)
    outs = []
    for launch in (lambda a, b: rec.cfg_dpm_step_guided(eu, em, ec, a, b, coef, st, G_TEXT, G_IMAGE, RESCALE),
                   lambda a, b: rec.cfg_dpm_step_pag(eu, em, ec, unread, a, b, coef, st, G_TEXT, G_IMAGE, 0.0, RESCALE),
                   lambda a, b: rec.cfg_dpm_step_guided(eu, None, ec, a, b, coef, st, G_TEXT, None, RESCALE),
                   lambda a, b: rec.cfg_dpm_step_guided(eu, unread, ec, a, b, coef, st, G_TEXT, G_TEXT, RESCALE)):
        a, b = c.put(x.clone()), c.put(xp.clone())
        launch(a, b)
        outs.append((a, b))
    rec.same_bits = [(outs[0][0], outs[1][0]), (outs[0][1], outs[1][1]), (outs[2][0], outs[3][0]), (outs[2][1], outs[3][1])]


add("step-substitutions-unread-inputs-are-nan", _step_substitutions)


def _product_steps(B, S):
    def run(c):
        shape = (B, 4, S, S)
        coef, st = _step_coef(c), _state(c, 1, STEP_ROWS)
        eu, em, ec, ep = (c.f(*shape) for _ in range(4))
        blend = dict(mask=_step_mask(c, B, S, S), known=c.f(*shape), noise=c.f(*shape))
        rng = c.put(_i32(STEP_RNG))
        c.rec.cfg_dpm_step_guided(eu, em, ec, c.f(*shape), c.f(*shape), coef, st, G_TEXT, G_IMAGE, RESCALE, **blend)
        c.rec.cfg_dpm_step_stochastic(eu, em, ec, c.f(*shape), c.f(*shape), coef, st, rng, G_TEXT, G_IMAGE, RESCALE, **blend)
        c.rec.cfg_dpm_step_pag(eu, em, ec, ep, c.f(*shape), c.f(*shape), coef, st, G_TEXT, G_IMAGE, G_PAG, RESCALE, rng=rng, **blend)
    return run


add("product-steps-16x4x64x64", _product_steps(16, 64))
add("product-steps-4x4x96x96", _product_steps(4, 96))


def _fusion_draw(c):
    n = 16
    forced = torch.full((n,), -1.0)
    forced[:4] = torch.tensor([0.0, 0.29, 0.5, 0.99])
    for state, only_last, fo in ((None, 0, None), ((STEP_ROWS - 1, STEP_ROWS), 1, forced), ((1, STEP_ROWS), 1, None)):
        c.rec.fusion_draw(None if state is None else _state(c, *state), c.put(_i32(STEP_RNG)), None if fo is None else c.put(fo), c.out_flat(n, 2),
                          n_layers=n, rule1=0.3, rule2=0.7, scale=2.0, only_last_step=only_last)


add("fusion-draw-16-layers", _fusion_draw)


# ============================================================================================================================== FreeU
def _freeu(c, B, h, w, cx, cs, *, b=1.5, s=0.2, sliced=False, flat_channels=False):
    """One pv_freeu_rows launch on strided inputs AND outputs (``Recorder.freeu`` always hands out contiguous outputs: the launch is recorded directly).
    ``sliced``: both inputs are column slices of one wider buffer.  ``flat_channels``: channel 0 of the skip is constant, channel 1 zero."""
    rows = B * h * w
    xs = c.randn(rows, max(cx, 1)) if cx else None
    sk = c.randn(rows, max(cs, 1)) + 0.5 if cs else None
    if flat_channels and cs:
        sk[:, 0], sk[:, 1] = 3.25, 0.0
    if sliced:
        buf = c.put(torch.cat([xs, sk], 1).to(F16), cx + cs + 8)
        x, skip = buf[:, :cx], buf[:, cx:]
    else:
        x = c.put(xs.to(F16), cx + 8) if cx else None
        skip = c.put(sk.to(F16), cs + 16) if cs else None
    xo = c.out(rows, cx, gap=24) if cx else None
    so = c.out(rows, cs, gap=8) if cs else None
    p = lambda t: t.data_ptr() if t is not None else None
    ld = lambda t: t.stride(0) if t is not None else 0
    c.rec._add(c.rec.lib.pv_freeu_rows, p(x), ld(x), cx, p(xo), ld(xo), float(b), p(skip), ld(skip), cs, p(so), ld(so), float(s), B, h, w, tag=("freeu_rows_kernel", 0.0, 0.0))


add("freeu-skip-cs8-2x2", lambda c: _freeu(c, 2, 2, 2, 0, 8, s=0.9))
add("freeu-skip-cs136-5x7", lambda c: _freeu(c, 2, 5, 7, 0, 136, s=0.2))                     # a second channel group with one live chunk; 35 pixels on 16 lanes
add("freeu-skip-cs16-4x6-constant-and-zero-channel", lambda c: _freeu(c, 2, 4, 6, 0, 16, s=2.0, flat_channels=True))      # even h: y = h / 2 is exact
add("freeu-x-cx16-2x2", lambda c: _freeu(c, 1, 2, 2, 16, 0))
add("freeu-x-cx48-5x7", lambda c: _freeu(c, 2, 5, 7, 48, 0, b=1.6))                            # 420 chunks: a second block, partly live
add("freeu-both-cx48-cs136-5x7", lambda c: _freeu(c, 2, 5, 7, 48, 136, b=1.5, s=0.9))
add("freeu-both-sliced-cx16-cs24-4x6", lambda c: _freeu(c, 2, 4, 6, 16, 24, sliced=True, flat_channels=True))


def _product_freeu(h, cs, b, s):
    def run(c):
        rows = 2 * h * h
        c.rec.freeu(c.put(c.randn(rows, 1280).to(F16)), c.put((c.randn(rows, cs) + 0.5).to(F16)), batch=2, h=h, w=h, b=b, s=s)
    return run


# the FreeU blocks of the SD-1.5 UNet (unet.UNetEngine: up block 0 at 8 x 8 pops three 1280-wide skips, up block 1 at 16 x 16 two of 1280 and one of 640)
add("product-freeu-8x8-c1280-skip1280", _product_freeu(8, 1280, 1.5, 0.9))
add("product-freeu-16x16-c1280-skip1280", _product_freeu(16, 1280, 1.6, 0.2))
add("product-freeu-16x16-c1280-skip640", _product_freeu(16, 640, 1.6, 0.2))


# ============================================================================================================================== resize / fp32 pointwise
def _resize(c, B, ch, h, w, oh, ow, *, ca=True, y=True, y_shift=False):
    x = c.f(B, ch, h, w)
    cav = c.put(torch.linspace(0.6, 1.4, B)) if ca else None           # a different ca[b] per sample
    yv = cbv = None
    if y:
        if y_shift:                                                   # ow % 4 == 0, y 4 bytes off a 16-byte boundary: the scalar kernel
            yv = c.f(B * ch * oh * ow + 1)[1:].view(B, ch, oh, ow)
            assert yv.data_ptr() % 16 == 4
        else:
            yv = c.f(B, ch, oh, ow)
        cbv = c.put(torch.linspace(-0.5, 0.7, B))
    c.rec.resize_bilinear_affine(x, (oh, ow), cav, yv, cbv, out=c.out_flat(B, ch, oh, ow))


add("resize-1x1-to-4x4", lambda c: (_resize(c, 2, 1, 1, 1, 4, 4), _resize(c, 2, 1, 1, 1, 4, 4, ca=False, y=False)))
add("resize-3x5-to-7x4-scalar", lambda c: (_resize(c, 2, 3, 3, 5, 7, 4), _resize(c, 2, 3, 3, 5, 7, 4, ca=False), _resize(c, 2, 3, 3, 5, 7, 4, y=False)))
add("resize-4x4-to-6x8-vector", lambda c: (_resize(c, 2, 3, 4, 4, 6, 8), _resize(c, 2, 3, 4, 4, 6, 8, ca=False, y=False), _resize(c, 2, 3, 4, 4, 6, 8, y=False)))
add("resize-8x8-identity", lambda c: (_resize(c, 2, 4, 8, 8, 8, 8, ca=False, y=False), _resize(c, 2, 4, 8, 8, 8, 8)))
add("resize-4x4-to-6x8-y-off-alignment", lambda c: _resize(c, 2, 3, 4, 4, 6, 8, y_shift=True))
add("product-resize-64-to-96", lambda c: _resize(c, 4, 4, 64, 64, 96, 96))


def _composite(c, h, w, alias):
    B, ch = 2, 3
    m = torch.rand(B, 1, h, w, generator=c.g)
    m.view(B, -1)[:, 0], m.view(B, -1)[:, 1] = 1.0, 0.0
    gen = c.f(B, ch, h, w, scale=1.5)
    c.rec.composite_clamp(gen, c.f(B, ch, h, w, scale=1.5), c.put(m), -1.0, 1.0, out=gen if alias else c.out_flat(B, ch, h, w))


add("composite-clamp-2x2", lambda c: _composite(c, 2, 2, False))
add("composite-clamp-6x6", lambda c: _composite(c, 6, 6, False))
add("composite-clamp-6x6-out-is-gen", lambda c: _composite(c, 6, 6, True))
for _n in (1, 35):
    add(f"clamp-n{_n}", lambda c, n=_n: c.rec.clamp_(c.f(2, 1, n, scale=2.0), -1.0, 1.0))
    add(f"affine-rows-n{_n}", lambda c, n=_n: (c.rec.affine_rows(c.f(2, 1, n), c.put(torch.tensor([0.7, -1.3])), out=c.out_flat(2, 1, n)),
                                               c.rec.affine_rows(c.f(2, 1, n), c.put(torch.tensor([0.7, -1.3])), c.f(2, 1, n), c.put(torch.tensor([0.4, 2.0])),
                                                                 out=c.out_flat(2, 1, n))))


# ============================================================================================================================== conditioning front ends
def _rows_mean(c, cols, count, group_rows, accumulate, groups=3):
    x = c.h((groups - 1) * group_rows + count, cols)
    y = c.h(groups, cols) if accumulate else c.out(groups, cols)
    c.rec.rows_mean(x, groups=groups, count=count, group_rows=group_rows, out=y, accumulate=accumulate)


add("rows-mean-cols8-count1", lambda c: _rows_mean(c, 8, 1, 1, False))
add("rows-mean-cols264-count9-gap-accumulate", lambda c: _rows_mean(c, 264, 9, 12, True))      # 33 chunks: a second block per group with one live chunk
add("rows-mean-cols8-count257-gap", lambda c: _rows_mean(c, 8, 257, 258, False))
add("rows-mean-cols264-count257-accumulate", lambda c: _rows_mean(c, 264, 257, 257, True))

#: fp32 values around every edge of the fp16 grid: the overflow threshold 65520 (the first value that rounds to infinity) and its neighbours, the
#: largest finite value, ties at the subnormal spacing 2^-24 (half of it rounds to even = 0), signed zeros, infinities
CAST_VALUES = (65520.0, 65519.996, 65504.0, 65536.0, -65520.0, 1e10, -7e4, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, -(2.0 ** -24), 2.0 ** -14,
               2.0 ** -14 - 2.0 ** -25, 0.0, -0.0, float("inf"), float("-inf"), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 0.1, -0.3)


def _casts(c):
    sp = torch.tensor(CAST_VALUES)
    wide = torch.cat([sp, c.randn(257 - sp.numel()) * 100.0])
    for t in (torch.tensor([65520.0]), wide):
        c.rec.cast_to_f16(c.put(t), out=c.out_flat(t.numel(), dtype=F16))
    h16 = torch.cat([sp.to(F16), c.randn(257 - sp.numel()).to(F16)])
    for t in (torch.tensor([-0.0], dtype=F16), h16):
        c.rec.cast_to_f32(c.put(t), out=c.out_flat(t.numel(), dtype=F32))


add("casts-n1-n257-grid-edges", _casts)
add("patchify-28px-patch14-kpad640", lambda c: c.rec.patchify(c.f(2, 3, 28, 28), batch=2, ch=3, img=28, patch=14, kpad=640))
add("clip-vision-embed-ntok5-dim8", lambda c: c.rec.clip_vision_embed(c.put(c.randn(2 * 4, 8).to(F16)), c.f(8), c.put(c.randn(5, 8)), batch=2, ntok=5, dim=8))


def _text_embed(c):
    B, S, dim, vocab = 2, 77, 8, 11
    tok, pos = c.put(c.randn(vocab, dim)), c.put(c.randn(S, dim))
    for E in (0, 1, 2):
        ids = torch.randint(0, vocab, (B, S), generator=c.g)
        ids[0, 1], ids[1, S - 1], ids[1, 3] = 0, 10, 10
        con = c.put(c.randn(B * E, dim).to(F16)) if E else None
        pidx = c.put(torch.tensor([0, S - E], dtype=torch.int64)) if E else None      # the placeholder at position 0 and at the last one that fits
        c.rec.clip_text_embed(c.put(ids), tok, pos, con, pidx, n_concept=E, batch=B, seq=S, dim=dim)


add("clip-text-embed-seq77-concepts-0-1-2", _text_embed)


# ============================================================================================================================== the training tape
# Single launches of the training tape's pointwise, reduction and weight-gradient launchers (no training plan is replayed).  The recorder's methods hand
# out contiguous outputs, so most launches are recorded directly: every operand that takes a leading dimension gets ld = cols + 8.
#: rows x cols of the launchers that walk 8-column chunks, 256 chunks a workgroup: one chunk; 165 chunks (no multiple of 256); 325 (a second workgroup)
PW_SHAPES = ((1, 8), (33, 40), (65, 40))
TRAIN_RNG = (0x9E3779B9, 0xDEADBEEF, 0x80000007)


def _dp(t):
    return t.data_ptr() if t is not None else None


def _ld(t):
    return t.stride(0) if t is not None else 0


def _xz(c, rows, cols, scale=2.0):
    """fp16 rows with exact zeros (and a negative zero) among them: the x > 0 branches of LeakyReLU / PReLU at 0."""
    t = c.randn(rows, cols, scale=scale)
    t.view(-1)[::7] = 0.0
    t.view(-1)[3::11] = -0.0
    return c.put(t.to(F16), cols + 8)


def _act_cases(c, backward):
    lib = c.rec.lib
    for rows, cols in PW_SHAPES:
        for act in range(5):
            x = _xz(c, rows, cols)
            if backward:
                dy, dx = c.h(rows, cols), c.out(rows, cols, gap=16)
                c.rec._add(lib.pv_act_backward, _dp(x), _ld(x), _dp(dy), _ld(dy), _dp(dx), _ld(dx), rows, cols, act)
            else:
                y = c.out(rows, cols, gap=16)
                c.rec._add(lib.pv_act_forward, _dp(x), _ld(x), _dp(y), _ld(y), rows, cols, act)


add("train-act-forward-every-activation", lambda c: _act_cases(c, False))
add("train-act-backward-every-activation", lambda c: _act_cases(c, True))


def _geglu_cases(c, backward):
    lib = c.rec.lib
    for rows, n in PW_SHAPES:
        h = c.h(rows, 2 * n, scale=2.0)
        if backward:
            dy, dh = c.h(rows, n), c.out(rows, 2 * n, gap=16)
            c.rec._add(lib.pv_geglu_backward, _dp(h), _ld(h), _dp(dy), _ld(dy), _dp(dh), _ld(dh), rows, n)
        else:
            out = c.out(rows, n)
            c.rec._add(lib.pv_geglu, _dp(h), _ld(h), _dp(out), _ld(out), rows, n)


add("train-geglu", lambda c: _geglu_cases(c, False))
add("train-geglu-backward", lambda c: _geglu_cases(c, True))


def _add_rows_cases(c):
    for rows, cols in PW_SHAPES:
        a = c.randn(rows, cols)
        b = c.randn(rows, cols)
        b.view(-1)[::3] *= 2.0 ** -14                        # exponents 14 and more apart: the fp32 sum itself rounds
        a.view(-1)[1::5] *= 1000.0
        a, b, out = c.put(a.to(F16), cols + 8), c.put(b.to(F16), cols + 16), c.out(rows, cols)
        c.rec._add(c.rec.lib.pv_add_rows_f16, _dp(a), _ld(a), _dp(b), _ld(b), _dp(out), _ld(out), rows, cols)


add("train-add-rows", _add_rows_cases)


def _col_affine_cases(c):
    for rows, cols in PW_SHAPES:
        for shift in (False, True):
            x, y = c.h(rows, cols), c.out(rows, cols)
            c.rec._add(c.rec.lib.pv_col_affine_f16, _dp(x), _ld(x), _dp(c.f(cols, scale=0.3, shift=1.0)), _dp(c.f(cols) if shift else None), _dp(y), _ld(y), rows, cols)


add("train-col-affine-with-and-without-shift", _col_affine_cases)


def _prelu_cases(c):
    slope = c.put(torch.tensor([0.3]))                          # no dyadic value: the product rounds in fp32
    for rows, cols in PW_SHAPES:
        for backward in (False, True):
            x, out = _xz(c, rows, cols), c.out(rows, cols)
            dy = c.h(rows, cols, gap=16) if backward else None
            c.rec._add(c.rec.lib.pv_prelu_f16, _dp(x), _ld(x), _dp(dy), _ld(dy), _dp(slope), _dp(out), _ld(out), rows, cols)


add("train-prelu-forward-and-backward", _prelu_cases)


def _softmax_bwd_cases(c):
    for rows, cols in PW_SHAPES:
        pm = c.put(torch.softmax(c.randn(rows, cols, scale=2.0), 1).to(F16), cols + 8)
        dp = c.h(rows, cols, gap=16)
        c.rec._add(c.rec.lib.pv_softmax_rows_backward, _dp(pm), _ld(pm), _dp(dp), _ld(dp), rows, cols, 0.3)


add("train-softmax-rows-backward", _softmax_bwd_cases)


def _dropout(c, x, rows, cols, copies, p, backward, add_t=None, site=5, rng=None):
    rng = c.put(_i32(TRAIN_RNG)) if rng is None else rng
    out = c.out(rows, cols if backward else copies * cols)
    c.rec._add(c.rec.lib.pv_dropout_f16, _dp(x), _ld(x), _dp(out), _ld(out), _dp(add_t), _ld(add_t), rows, cols, copies, float(p), _dp(rng), site, int(backward))
    return out


def _dropout_cases(c):
    for (rows, cols), p, copies in zip(PW_SHAPES * 2, (0.0, 0.1, 0.0, 0.1, 0.0, 0.1), (1, 3, 3, 1, 3, 3)):
        _dropout(c, c.h(rows, cols), rows, cols, copies, p, False)
        _dropout(c, c.h(rows, copies * cols), rows, cols, copies, p, True)
        _dropout(c, c.h(rows, copies * cols), rows, cols, copies, p, True, add_t=c.h(rows, cols, gap=16))


def _dropout_masks(c):
    """p = 0.5 (a scale of exactly 2) on all-ones: the backward of ones is 2 x the number of kept copies, and so is the sum over the copies (a p = 0
    backward: keep everything, scale 1) of the forward's own output - every value a small even integer, exact in fp16: the two agree bit for bit."""
    rows, cols, copies = 33, 40, 3
    rng = c.put(_i32(TRAIN_RNG))
    fwd = _dropout(c, c.put(torch.ones(rows, cols, dtype=F16), cols + 8), rows, cols, copies, 0.5, False, rng=rng)
    bwd = _dropout(c, c.put(torch.ones(rows, copies * cols, dtype=F16), copies * cols + 8), rows, cols, copies, 0.5, True, rng=rng)
    total = _dropout(c, fwd, rows, cols, copies, 0.0, True, rng=rng)
    c.rec.same_bits = [(bwd, total)]


add("train-dropout-p-copies-forward-backward-add", _dropout_cases)
add("train-dropout-backward-is-the-sum-of-the-forward-masks", _dropout_masks)


def _maxpool_cases(c):
    for batch, h, w, ch in ((1, 2, 2, 8), (2, 4, 6, 16)):
        for backward in (False, True):
            x = c.put((torch.randint(0, 3, (batch * h * w, ch), generator=c.g) * 0.5 - 0.5).to(F16))          # three values: ties in most windows
            dy = c.put(c.randn(batch * (h // 2) * (w // 2), ch).to(F16)) if backward else None
            out = c.out(batch * h * w if backward else batch * (h // 2) * (w // 2), ch, gap=0)
            c.rec._add(c.rec.lib.pv_maxpool2x2, _dp(x), _dp(dy), _dp(out), batch, h, w, ch)


add("train-maxpool2x2-ties", _maxpool_cases)


def _dilate_pool_cases(c):
    B, h, w = 2, 3, 5
    for ch in (8, 24):
        x, z = c.h(B * h * w, ch), c.out(B * 4 * h * w, ch, gap=0)
        c.rec._add(c.rec.lib.pv_dilate2x, _dp(x), _ld(x), _dp(z), B, h, w, ch)
        for with_add in (False, True):
            g, ad = c.put(c.randn(B * 4 * h * w, ch).to(F16)), (c.h(B * h * w, ch) if with_add else None)
            c.rec._add(c.rec.lib.pv_pool2x_sum, _dp(g), _dp(ad), _ld(ad), _dp(c.out(B * h * w, ch, gap=0)), B, h, w, ch)


add("train-dilate2x-pool2x-3x5", _dilate_pool_cases)


def _gather_cases(c):
    B, seq, n_e, dim = 3, 7, 3, 264
    x = c.h(B * seq, dim)
    idx = c.put(torch.tensor([seq - 1, -1, 2], dtype=I32))       # the rows behind seq - 1 and the row in front of 0 are outside their sample: 0
    c.rec._add(c.rec.lib.pv_gather_rows_f32, _dp(x), _ld(x), _dp(idx), _dp(c.out_flat(B * n_e * dim)), B, seq, n_e, dim, 0.5)
    x1 = c.h(2 * seq, 8)
    c.rec._add(c.rec.lib.pv_gather_rows_f32, _dp(x1), _ld(x1), _dp(c.put(torch.tensor([0, seq - 1], dtype=I32))), _dp(c.out_flat(2 * 8)), 2, seq, 1, 8, 1.0)


add("train-gather-rows-outside-rows", _gather_cases)


def _sign_clamp_cases(c):
    for n in (1, 257):
        x = c.randn(n)
        x[:4] = torch.tensor([0.0, -0.0, 1.0, -1.0])[:n]
        c.rec.sign(c.put(x), 0.25)
        y = c.randn(n) * 1.5
        y[:5] = torch.tensor([-1.0, 1.0, 0.0, -1.0000001, 0.99999994])[:n]       # exactly lo and hi (outside), 0, and their fp32 neighbours
        c.rec.clamp_mask(c.put(y), c.f(n), -1.0, 1.0)


add("train-sign-clamp-mask-n1-n257", _sign_clamp_cases)


def _transpose_cases(c):
    for rows, cols, rp, ldo in ((33, 40, 64, 64), (7, 8, 7, 7), (33, 40, 33, 48)):
        x, out = c.h(rows, cols), c.out(cols, rp, gap=ldo - rp)
        c.rec._add(c.rec.lib.pv_transpose_f16, _dp(x), _ld(x), rows, cols, _dp(out), ldo, rp)


add("train-transpose-rows-pad", _transpose_cases)


def _reduce_blocks_cases(c):
    for nblk in (1, 7, 8, 9, 31, 32, 33, 57):
        for inner in (1, 33):
            c.rec._add(c.rec.lib.pv_reduce_blocks, _dp(c.put(c.randn(nblk, inner))), nblk, inner, 0.25, _dp(c.out_flat(inner)))


add("train-reduce-blocks-both-unroll-tails", _reduce_blocks_cases)


def _colsum_cases(c):
    c.rec.colsum(c.h(130, 257))
    x = c.h(5, 8)
    c.rec._add(c.rec.lib.pv_colsum_f16, _dp(x), _ld(x), 5, 8, _dp(c.out_flat(4 * 8)), 4, _dp(c.out_flat(8)))       # rows_per_block 2: block 3 owns no row


add("train-colsum-130x257-and-an-empty-block", _colsum_cases)


def _reduce_mean_cases(c):
    for n in (1, 255, 4097):                                     # 4097: two partials of 256 threads, a grid-stride loop of nine trips
        for dt in (F32, F16):
            for mode in ("mean", "abs", "mse"):
                a = c.put((c.randn(n) + 0.25).to(dt))
                c.rec.reduce_mean(a, c.put(c.randn(n).to(dt)) if mode == "mse" else None, mode=mode, out=c.out_flat(1))
        c.rec.reduce_sumsq(c.f(n), out=c.out_flat(1), scale=0.5)


add("train-reduce-mean-sumsq-modes-types-n", _reduce_mean_cases)


def _gray_cases(c):
    B = 2
    for h, w, S in ((5, 5, 8), (9, 9, 4), (6, 6, 6), (7, 5, 4)):
        x = c.put(c.randn(B, 3 * h * w), 3 * h * w + 8)           # an image stride larger than the image
        c.rec._add(c.rec.lib.pv_gray_resize, _dp(x), _ld(x), _dp(c.out_flat(B * S * S)), B, h, w, S, 0.5, -1.0)
        dy = c.put(c.randn(B, S * S), 3 * S * S)                  # channel 0 of a 3-channel buffer
        c.rec._add(c.rec.lib.pv_gray_resize_backward, _dp(dy), _ld(dy), _dp(c.out_flat(B * 3 * h * w)), B, h, w, S, 0.5)


add("train-gray-resize-and-backward", _gray_cases)


def _cosine_cases(c):
    B = 3
    for dim in (8, 100, 512):
        for target in (1.0, -1.0):
            for grad in (False, True):
                e1 = c.randn(B, dim)
                e2 = 0.9 * e1 + 0.3 * c.randn(B, dim)              # cosines near +-0.95: far from the max(0, cos) branch point
                e2[1] = -e2[1]
                ls, de2 = c.out_flat(B), (c.out(B, dim, gap=0) if grad else None)
                c.rec._add(c.rec.lib.pv_cosine_embedding_loss, _dp(c.put(e1.to(F16))), _dp(c.put(e2.to(F16))), B, dim, target, 4.0, _dp(ls), _dp(de2))


add("train-cosine-embedding-loss-dims-targets", _cosine_cases)


def _ln_bwd(c, rows, cols, *, act=0, affine=False, rpw=1, ldx=None, with_add=False, dy_group=1, dy_skip=0, dy_scale=1.0):
    from photoverse_amd._lib import LayerNormBwdParams
    gap = 8 if cols % 8 == 0 else 4
    x = c.put((c.randn(rows, cols) * 1.5 + 0.3).to(F16), ldx or cols + gap)
    dy = c.put(c.randn((rows - 1) // max(dy_group, 1) + 1, cols).to(F16), cols + 2 * gap)
    dx = c.out(rows, cols, gap=gap)
    gam, bet = c.f(cols, scale=0.2, shift=1.0), c.f(cols, scale=0.1)
    ad = c.put(c.randn(rows, cols).to(F16), cols + 2 * gap) if with_add else None
    nblk = (rows + 4 * rpw - 1) // (4 * rpw)
    part = c.out(nblk, 2 * cols, F32, gap=0) if affine else None
    p = LayerNormBwdParams(_dp(x), _ld(x), _dp(dy), _ld(dy), _dp(dx), _ld(dx), _dp(gam), _dp(bet), _dp(part), rows, cols, 1e-5, act, dy_group, dy_skip, dy_scale, rpw,
                           _dp(ad), _ld(ad))
    c.rec._add(c.rec.lib.pv_layernorm_backward, p)
    return part, nblk


def ln_bwd_full_workgroup(cols: int) -> int:
    """Rows of one workgroup of the vector form the launcher picks for ``cols``: 4 waves of 64 / LPR rows (the header's dispatch by cols / 8)."""
    nch = cols // 8
    lpr = 8 if nch <= 40 else 16 if nch <= 96 else 32 if nch <= 160 else 64
    return 4 * 64 // lpr


#: both sides of every threshold of the vector dispatch, its narrowest and widest rows, and a width inside the first instantiation
LN_BWD_COLS = (8, 200, 320, 328, 640, 648, 768, 776, 1024, 1032, 1280, 1288, 2048)


def _ln_bwd_vector(c):
    for i, cols in enumerate(LN_BWD_COLS):
        _ln_bwd(c, ln_bwd_full_workgroup(cols) + 1, cols, act=3 if i % 2 == 0 else 0, with_add=i % 3 == 0)


def _ln_bwd_scalar_affine(c):
    _ln_bwd(c, 5, 324, act=3)                                    # no multiple of 8: the one-wave-per-row kernel
    _ln_bwd(c, 5, 320, act=0, ldx=321, with_add=True)            # a row stride that is no multiple of 8
    part, nblk = _ln_bwd(c, 9, 40, act=3, affine=True)           # rows_per_wave 1: two blocks and one row
    c.rec._add(c.rec.lib.pv_reduce_blocks, _dp(part), nblk, 2 * 40, 1.0, _dp(c.out_flat(2 * 40)))
    _ln_bwd(c, 2053, 8, act=3, affine=True, rpw=2, with_add=True)       # rows_per_wave 2: 256 blocks of 8 rows and one of 5
    _ln_bwd(c, 7, 200, act=0, affine=True)


def _ln_bwd_grouped(c):
    _ln_bwd(c, 33, 320, act=3, dy_group=5, dy_skip=1, dy_scale=0.25)                       # a vector instantiation; the last group has three rows
    _ln_bwd(c, 33, 40, act=3, affine=True, dy_group=5, dy_skip=1, dy_scale=0.25, with_add=True)


add("train-layernorm-backward-vector-thresholds", _ln_bwd_vector)
add("train-layernorm-backward-scalar-and-affine", _ln_bwd_scalar_affine)
add("train-layernorm-backward-dy-group-skip-scale", _ln_bwd_grouped)


def _wgrad_cases(c):
    """The launch pair ``Recorder.wgrad`` records (the slabs, then their pv_reduce_blocks with the scale), with the slab height given: 64-row slabs for the
    small shapes; (1025, 8, 136) in slabs of 1024 rows: two slabs, the last one of a single row."""
    for m, n, k, rps in ((7, 8, 8, 64), (65, 136, 200, 64), (1025, 8, 136, 1024)):
        dy = c.put(c.randn(m, n + 8).to(F16), n + 16)[:, 8:]     # a column slice: the row gap holds NaN behind it and 8 live columns in front
        x = c.h(m, k)
        nsplit = (m + rps - 1) // rps
        part = c.rec.empty((nsplit, n, k), F32)
        c.rec._add(c.rec.lib.pv_wgrad_tn, _dp(dy), _ld(dy), _dp(x), _ld(x), m, n, k, _dp(part), nsplit, rps, tag=("pv_wgrad_tn", 0.0, 0.0))
        c.rec._add(c.rec.lib.pv_reduce_blocks, _dp(part), nsplit, n * k, 0.5, _dp(c.out_flat(n * k)))


add("train-wgrad-tn-slabs-and-their-sum", _wgrad_cases)


#: Instantiations no argument and no per-call switch can select: the only symbols the dispatch sweep may leave unaudited
EXEMPT = {
    "big_tile_kernel<false, false, 4, 1, false>": "the 128-row form of the 256 x 320 tile: behind PV_GEMM_BIG128, read once per process",
    "big_tile_kernel<true, false, 4, 1, false>": "the same with column statistics: behind PV_GEMM_BIG128, read once per process",
    "attn_kernel<40, 4, false>": "d = 40 without the LDS-DMA ring: needs PV_ATTN_NO_DMA (read once per process) or a K / V operand of 2 GiB or more",
    "attn_kernel<40, 2, false>": "d = 40 without the LDS-DMA ring: needs PV_ATTN_NO_DMA (read once per process) or a K / V operand of 2 GiB or more",
    **{f"attn8_kernel<{v}>": "a non-default form of the 8-wave kernel: PV_ATTN8 selects it, kept for the measurements of EXPERIMENTS.md"
       for v in (0, 1, 9, 13, 33, 49, 73, 201, 225, 241, 481)},
}
#: switches read once per process that change which kernel (or workgroup shape) a launch takes; the suite runs with none of them set
PROCESS_SWITCHES = ("PV_GEMM_BIG128", "PV_XF_ROWS", "PV_ATTN_NO_DMA", "PV_ATTN_NQ", "PV_GEMM_MI2", "PV_GEMM_TPW")


# ============================================================================================================================== dispatch sweep
SWEEP_M = (1, 65, 130, 257, 4096, 65536, 131073)
SWEEP_BIG_MIN = (0, 1, 128, -1)


def _sweep_gemm(sym: set):
    probe = gemm_symbol
    for big in SWEEP_BIG_MIN:
        for M in SWEEP_M:
            for N in (128, 160, 256, 320, 640, 1024, 1280):
                for K in (64, 192, 320, 640, 1280):
                    for c1 in (0, K):
                        base = _lin_fields(M, N, K, big_tile_min=big, c1=c1, lda1=c1, a1=0x1000 if c1 else 0, hout=100)
                        for extra in ({}, dict(out_f32=1), dict(colstats=0x1000), dict(geglu=1, ldc=N // 2), dict(ln_rowsum=0x1000), dict(geglu=1, ldc=N // 2, ln_rowsum=0x1000),
                                      dict(residual=0x1000, ldr=N, bias=0x1000, act=1, rowadd=0x1000, rowadd_ld=N)):
                            for sk in (0, 2, 3):
                                sym.add(probe(**{**base, **extra}, splitk=sk, splitk_ws=0x1000 if sk else 0))
        geos = [(2, 5, 7), (1, 10, 10), (1, 5, 5), (1, 4, 64), (2, 4, 64), (1, 8, 32), (2, 8, 32), (16, 64, 64), (16, 32, 32), (16, 16, 16), (4, 96, 96), (4, 24, 24)]
        for patch in (None, "0", "1"):
            with environment({} if patch is None else {"PV_CONV_PATCH": patch}, folds=False):
                for b, h, w in geos:
                    for stride, up, pad in ((1, 0, 1), (2, 0, 1), (2, 0, 0), (1, 1, 1)):
                        hl, wl = (2 * h, 2 * w) if up else (h, w)
                        ho, wo = ((hl + (2 if pad else 1) - 3) // 2 + 1, (wl + (2 if pad else 1) - 3) // 2 + 1) if stride == 2 else (hl, wl)
                        for cin, c1 in ((64, 0), (64, 64), (128, 0), (320, 0), (640, 640)):
                            for N in (128, 160, 320, 640):
                                base = dict(c0=cin, c1=c1, lda0=cin, lda1=c1, a1=0x1000 if c1 else 0, N=N, ldc=N, M=b * ho * wo, taps=9, batch=b, hin=h, win=w, hout=ho, wout=wo,
                                            stride=stride, upsample=up, pad=pad, big_tile_min=big)
                                for extra in ({}, dict(colstats=0x1000), dict(a_norm=0x1000, a_norm_act=1), dict(a_norm=0x1000, colstats=0x1000), dict(out_f32=1)):
                                    for sk in (0, 2, 3, 5, 8):
                                        sym.add(probe(**{**base, **extra}, splitk=sk, splitk_ws=0x1000 if sk else 0))


def _sweep_attention(sym: set):
    for env in ({}, {"PV_ATTN8_MIN": "1"}, {"PV_ATTN8": "-1"}, {"PV_ATTN8": "-1", "PV_ATTN8_MIN": "1"}):
        with environment(env, folds=False):
            for d in (40, 64, 80, 160):
                for batch, heads in ((1, 2), (2, 8), (16, 8), (64, 8), (128, 8)):
                    for nq in (1, 65, 257, 600, 1024, 4096, 9216):
                        for nk in {1, 77, nq}:
                            for causal in (0, 1):
                                ld = 3 * heads * d + 8
                                sym.add(attn_symbol(batch=batch, heads=heads, nq=nq, nk=nk, d=d, causal=causal, ldq=ld, ldk=ld, ldv=ld, ldo=heads * d, lse=0))


DISPATCHED = ("gemm_conv_kernel<", "big_tile_kernel<", "attn_kernel<", "attn8_kernel<")
_SWEPT: Optional[frozenset] = None


def swept_symbols() -> frozenset:
    """Every kernel symbol ``pv_gemm_conv_kernel_info`` / ``pv_attention_kernel_info`` name over a grid of contract-valid parameter blocks (M, every N /
    K family, taps, stride, upsample, split-K, big_tile_min, the per-call switches) - no GPU needed.  Blocks the library rejects count for nothing."""
    global _SWEPT
    if _SWEPT is None:
        sym: set = set()
        _sweep_gemm(sym)
        _sweep_attention(sym)
        sym.discard("")
        _SWEPT = frozenset(sym)
    return _SWEPT


def by_name(name: str) -> Case:
    return next(c for c in CASES if c.name == name)
