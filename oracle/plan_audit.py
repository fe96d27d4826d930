"""Replay a recorded launch plan (``photoverse_amd.ops.Recorder``) one launch at a time against ``oracle.abi_ref``.

Per call: every pointer field is resolved to a strided view of a tensor the plan holds (an address outside them, or an extent that runs past
its tensor, is a use-after-free / out-of-bounds plan and fails with the plan, call index and field named); outputs are poisoned with NaN
(unless an input overlaps them); the single call runs on the current stream; every output is compared element by element with the fp64
reference and in aggregate; the bytes of the outputs' tensors outside the described extents must be unchanged; column statistics must match
sums over the kernel's own output; a second run from the restored inputs must give bit-identical outputs.  The plan then goes on from the
kernel's own results, so that every later launch sees the product's real activations.
"""
from __future__ import annotations

import bisect
import ctypes as C
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch

from . import abi_ref as A


class AuditError(AssertionError):
    pass


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    n = b.norm().item()
    return (a - b).norm().item() / n if n > 0 else (a - b).norm().item()


def held_tensors(*objs) -> List[torch.Tensor]:
    """Every tensor the recorders (and their nested recorders) hold."""
    out, seen = [], set()

    def walk(o):
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            out.append(o)
        elif hasattr(o, "keep") and hasattr(o, "calls"):
            for k in o.keep:
                walk(k)
        elif isinstance(o, (list, tuple)):
            for k in o:
                walk(k)
    for o in objs:
        walk(o)
    return out


class Pool:
    """Address -> held storage."""

    def __init__(self, tensors):
        st = {}
        for t in tensors:
            if t.is_cuda:
                s = t.untyped_storage()
                st[s.data_ptr()] = (s.data_ptr(), s.data_ptr() + s.nbytes(), s, t.device)
        self.ent = sorted(st.values(), key=lambda e: e[0])
        self.starts = [e[0] for e in self.ent]

    def find(self, addr: int, nbytes: int):
        i = bisect.bisect_right(self.starts, addr) - 1
        if i < 0:
            return None
        # nested / overlapping storages do not occur (one storage per allocation); take the containing one
        lo, hi, s, dev = self.ent[i]
        if addr >= hi:
            return None
        return (lo, hi, s, dev) if addr + nbytes <= hi else (lo, hi, None, dev)


def _isz(dt):
    return torch.empty((), dtype=dt).element_size()


def make_view(pool: Pool, addr: int, buf: A.Buf, where: str):
    isz = _isz(buf.dtype)
    ld = buf.ld if buf.ld else buf.cols
    ext = ((buf.rows - 1) * ld + buf.cols) * isz if buf.rows > 0 and buf.cols > 0 else 0
    hit = pool.find(addr, ext)
    if hit is None:
        raise AuditError(f"{where}: address {addr:#x} lies in no tensor the plan holds (use after free?)")
    lo, hi, s, dev = hit
    if s is None:
        raise AuditError(f"{where}: extent {buf.rows} x {buf.cols} (ld {ld}, {ext} bytes) runs past its tensor ({hi - addr} bytes left)")
    if (addr - lo) % isz:
        raise AuditError(f"{where}: misaligned address for {buf.dtype}")
    flat = torch.empty(0, dtype=buf.dtype, device=dev).set_(s, 0, ((hi - lo) // isz,), (1,))
    return flat.as_strided((buf.rows, buf.cols), (ld, 1), (addr - lo) // isz), (lo, s)


def compare(exp: Dict[str, A.Expect], got: Dict[str, torch.Tensor]):
    """(failures, worst element error / bound, worst aggregate rel-L2 / bound) of the outputs ``got`` against the references ``exp``.
    Aggregate bound: ``1.5 rel_l2(round(ref), ref) + 1e-6 + agg_extra`` - as good as rounding the exact answer to the output type, plus the
    documented intermediates' allowance - and never above the launcher's kernel-test tolerance (``Expect.cap``)."""
    fails, worst, worst_agg = [], 0.0, 0.0
    for k, e in exp.items():
        if e.after is not None:
            e = e.after(got)
        g = (e.derive(got) if e.derive is not None else got[k]).double()
        if e.store is None:
            if not torch.equal(g, e.ref):
                fails.append(f"field {k}: {(g != e.ref).sum().item()} elements differ from the exact reference")
            continue
        fin = torch.isfinite(e.ref)
        if not bool(torch.isfinite(g[fin]).all()):
            fails.append(f"field {k}: {(~torch.isfinite(g[fin])).sum().item()} non-finite (unwritten?) elements")
            continue
        ratio = torch.where(fin, (g - e.ref).abs() / e.bound, torch.zeros_like(g))
        r = ratio.max().item() if ratio.numel() else 0.0
        worst = max(worst, r)
        if r > 1.0:
            rr, cc = divmod(int(ratio.argmax()), g.shape[1])
            fails.append(f"field {k}: error {r:.3g} x its bound (worst at row {rr}, col {cc})")
        rq = e.rounded if e.rounded is not None else e.ref.to(e.store).double()
        agg_b = 1.5 * rel_l2(rq, e.ref) + 1e-6 + e.agg_extra
        if e.cap is not None:
            agg_b = min(agg_b, e.cap)
        ra = rel_l2(g, e.ref) / agg_b
        worst_agg = max(worst_agg, ra)
        if ra > 1.0:
            fails.append(f"field {k}: rel-L2 {rel_l2(g, e.ref):.3e} > bound {agg_b:.3e}")
    return fails, worst, worst_agg


def written_mask(storage, views) -> torch.Tensor:
    """Byte mask of ``storage`` covering the [rows, cols] extents of ``views`` (those that live in it)."""
    sp = storage.data_ptr()
    m = torch.zeros(storage.nbytes(), dtype=torch.bool, device=storage.device)
    for t in views:
        if t.untyped_storage().data_ptr() != sp or t.numel() == 0:
            continue
        isz = t.element_size()
        m.as_strided((t.shape[0], t.shape[1] * isz), (t.stride(0) * isz, 1), t.data_ptr() - sp).fill_(True)
    return m


def storage_bytes(storage) -> torch.Tensor:
    return torch.empty(0, dtype=torch.uint8, device=storage.device).set_(storage, 0, (storage.nbytes(),), (1,))


def changed_outside(before: torch.Tensor, storage, views) -> int:
    """Bytes of ``storage`` outside the extents of ``views`` that differ from the snapshot ``before``."""
    m = written_mask(storage, views)
    return int((storage_bytes(storage)[~m] != before[~m]).sum().item())


class Params:
    """Attribute view of a launch's arguments: the struct's fields, then the positional arguments by name."""

    def __init__(self, struct, extra: Dict[str, object]):
        object.__setattr__(self, "_s", struct)
        object.__setattr__(self, "_x", extra)

    def __getattr__(self, k):
        if k in self._x:
            v = self._x[k]
            return 0 if v is None else v
        return getattr(self._s, k)


def _flags(name, p) -> str:
    g = lambda k: getattr(p, k, 0) or 0
    if name == "pv_gemm_conv":
        f = [f"taps={p.taps}"]
        f += [k for k, c in (("stride2", p.taps == 9 and p.stride == 2), ("up", g("upsample")), ("pad0", p.taps == 9 and p.pad == 0),
                             ("a1", g("a1")), ("rowadd", g("rowadd")), ("rowadd/img", g("rowadd_ld")), ("res", g("residual")),
                             ("f32", g("out_f32")), ("geglu", g("geglu")), ("colstats", g("colstats")), ("ln", g("ln_rowsum")),
                             ("anorm", g("a_norm"))) if c]
        if p.act:
            f.append(f"act={p.act}")
        return " ".join(f)
    if name in ("pv_cfg_dpm_step_guided", "pv_cfg_dpm_step_stochastic", "pv_cfg_dpm_step_pag"):
        three, pag = A.step_reads(p)
        return " ".join(k for k, c in (("three-forward", three), ("pag", pag), ("rescale", p.rescale > 0), ("mask", g("mask")), ("rng", g("rng"))) if c)
    if name in A.TRAINING:
        f = [f"act={A.ACT_NAMES.get(p.act, p.act)}"] if name in ("pv_act_forward", "pv_act_backward", "pv_layernorm_backward") else []
        f += [k for k in ("backward", "add", "shift", "dy", "de2", "dgb_partial", "is_f16") if g(k) and not (k == "dy" and name not in ("pv_prelu_f16", "pv_maxpool2x2"))]
        f += [f"{k}={g(k)}" for k in ("copies", "mode", "nsplit", "rows_per_wave", "dy_group", "n_e") if g(k) and (k != "copies" or g(k) > 1)]
        if name == "pv_layernorm_backward":
            f.append("vector" if not g("dgb_partial") and p.cols % 8 == 0 and (p.ldx | p.lddy | p.lddx | (p.ldadd if g("add") else 0)) % 8 == 0 else "scalar")
        if name == "pv_dropout_f16":
            f.append(f"p={p.p:g}")
        if name == "pv_cosine_embedding_loss":
            f.append(f"target={p.target:g}")
        return " ".join(f)
    keys = {"pv_freeu_rows": ("x", "skip"), "pv_resize_bilinear_affine_f32": ("ca", "y"), "pv_affine_rows_f32": ("y",), "pv_rows_mean": ("accumulate",),
            "pv_clip_text_embed": ("n_concept",),
            "pv_attention": ("causal", "lse"), "pv_cross_attention": ("vnorm", "fusion"), "pv_cross_attention_lnq": ("ln", "vnorm", "fusion"),
            "pv_cross_attention_fused": ("ln", "fusion"), "pv_row_gemm": ("ln", "geglu", "x_norm"), "pv_groupnorm_apply": ("act",),
            "pv_layernorm": ("act",)}.get(name, ())
    f = [k for k in keys if g(k)]
    if name in ("pv_attention", "pv_cross_attention", "pv_cross_attention_lnq", "pv_cross_attention_fused"):
        f.append(f"d={p.d}")
    return " ".join(f)


class Auditor:
    def __init__(self, lib):
        self.lib = lib
        self.rows: Dict[tuple, dict] = {}
        self.kv: Dict[int, tuple] = {}          # kimg address -> the K / V rows pv_xattn_pack_kv read
        self.audited = 0
        self._wo_slot: Dict[int, list] = {}

    def wo_slot(self, C_: int):
        if C_ not in self._wo_slot:
            self._wo_slot[C_] = [self.lib.pv_xattn_fused_wo_slot(s) for s in range(C_)]
        return self._wo_slot[C_]

    # ---------------------------------------------------------------------------------------------------------------------------------
    def audit(self, plan: str, rec, holders=()) -> int:
        """Audit every call of ``rec`` in order (returns the number of calls that completed every check); ``holders``: further recorders of the same plan whose tensors ``rec``'s calls may address
        (the recorders of one engine / loop share their buffers)."""
        pool = Pool(held_tensors(rec, *holders))
        stream = torch.cuda.current_stream().cuda_stream
        before = self.audited
        for i, (fn, args) in enumerate(rec.calls):
            tag = rec.tags[i][0] if i < len(rec.tags) else fn.__name__
            self._one(plan, i, fn, args, tag, pool, stream)
        return self.audited - before

    def _one(self, plan, i, fn, args, tag, pool, stream):
        name = fn.__name__
        where = f"{plan} call {i} ({name}, {tag})"
        if name not in A.LAYOUT:
            raise AuditError(f"{where}: no reference for this launcher")
        if args and isinstance(args[0], type(C.byref(C.c_int()))):
            extra = dict(zip(A.ARGS.get(name, ()), args[1:]))
            p = Params(args[0]._obj, extra)
        else:
            p = Params(None, dict(zip(A.ARGS[name], args)))
        L = dict(A.LAYOUT[name](p))
        v, base = {}, {}

        def resolve(k, buf):
            addr = getattr(p, k)
            if not addr:
                return
            v[k], base[k] = make_view(pool, addr, buf, f"{where}, field {k}")

        # a field whose extent depends on device contents (the step index, the token ids) is resolved after the buffer that holds them (A.DEPENDENT)
        dep = A.DEPENDENT.get(name)
        if dep is not None and L.get(dep[0]) is not None:
            first_k, dep_k, extent, row = dep
            resolve(first_k, L[first_k])
            if first_k in v:
                L[dep_k] = extent(p, v[first_k])
        for k, buf in L.items():
            if k not in v and buf is not None:
                resolve(k, buf)
        if dep is not None and dep[3] and dep[1] in v:
            v[dep[1]] = v[dep[1]][:, A.step_index(v[dep[0]]) * dep[3]:][:, :dep[3]]
        if name == "pv_cross_attention_fused" and p.kimg not in self.kv:
            raise AuditError(f"{where}: kimg {p.kimg:#x} was not built by an audited pv_xattn_pack_kv")

        roles = {k: L[k].role for k in v}
        outs = [k for k in v if roles[k] in ("out", "inout", "opaque")]
        ins = [k for k in v if roles[k] in ("in", "inout")]
        # checked sub-regions of scratch buffers: (mean, rstd) at partial[b][0][g]
        checks = {}
        if name in ("pv_groupnorm_stats", "pv_groupnorm_stats_from_colstats", "pv_groupnorm_scale_shift"):
            checks["partial[:, 0]"] = v["partial"][::p.splits]

        def ext(k):
            t = v[k]
            lo = t.data_ptr()
            return lo, lo + ((t.shape[0] - 1) * t.stride(0) + t.shape[1]) * t.element_size()
        overlap = lambda a, b: ext(a)[0] < ext(b)[1] and ext(b)[0] < ext(a)[1]

        # reference first, from the pristine inputs (the kernel may write in place)
        kw = {}
        if name == "pv_cross_attention_fused":
            kw = dict(kv=self.kv[p.kimg], wo_slot=self.wo_slot(p.heads * p.d))
        exp = A.REF[name](p, v, **kw)
        if name == "pv_xattn_pack_kv":
            self.kv[p.kimg] = tuple(None if k not in v else v[k].clone() for k in ("kt", "vt", "kip", "vip"))

        poison = [k for k in outs if roles[k] == "out" and not any(overlap(k, j) for j in ins)]
        inout_snap = {k: v[k].clone() for k in v if roles[k] == "inout" or (roles[k] == "out" and k not in poison)}
        stores = {}
        for k in v:
            if roles[k] in ("out", "inout", "opaque", "scratch"):
                lo, s = base[k]
                stores.setdefault(s.data_ptr(), (s, lo, v[k].device))
        snaps = {sp: storage_bytes(s).clone() for sp, (s, lo, dev) in stores.items()}
        wviews = [v[k] for k in v if roles[k] in ("out", "inout", "opaque", "scratch")]

        def poison_all():
            for k in poison:
                if v[k].dtype.is_floating_point:
                    v[k].fill_(float("nan"))
            for k, t in checks.items():
                t.fill_(float("nan"))
            for k, t in inout_snap.items():
                v[k].copy_(t)
            # the bytes around are the pre-call bytes again
            for sp, (s, lo, dev) in stores.items():
                m = written_mask(s, wviews)
                flat = storage_bytes(s)
                flat[~m] = snaps[sp][~m]

        def launch():
            rc = fn(*args, stream)
            if rc != 0:
                raise AuditError(f"{where}: launch failed with hipError {rc}")
            torch.cuda.synchronize()

        poison_all()
        launch()
        first = {k: v[k].clone() for k in outs}
        first.update({k: t.clone() for k, t in checks.items()})
        fails = []
        # bytes around the outputs
        for sp, (s, lo, dev) in stores.items():
            bad = changed_outside(snaps[sp], s, wviews)
            if bad:
                fails.append(f"{bad} bytes changed outside the described output extents")
        got = dict(v)
        got.update(checks)
        f2, worst, worst_agg = compare(exp, got)
        fails += f2
        # determinism: the same call again from the restored inputs
        poison_all()
        launch()
        for k, t in first.items():
            now = got[k] if k in got else v[k]
            if not torch.equal(now.contiguous().view(torch.uint8) if now.dtype != torch.uint8 else now, t.contiguous().view(torch.uint8)):
                fails.append(f"field {k}: a second run gave different bits")
        if fails:
            raise AuditError(f"{where}: " + "; ".join(fails))
        key = (plan, name, tag, int(getattr(p, "splitk", 0) or 0) if name == "pv_gemm_conv" else 0, _flags(name, p))
        row = self.rows.setdefault(key, dict(n=0, worst=0.0, agg=0.0))
        row["n"] += 1
        row["worst"] = max(row["worst"], worst)
        row["agg"] = max(row["agg"], worst_agg)
        self.audited += 1

    def table(self) -> str:
        lines = [f"{'plan':<12} {'launcher':<34} {'kernel':<44} {'splitk':>6} {'n':>5} {'err/bound':>9} {'agg/bound':>9}  flags"]
        for (plan, name, tag, sk, fl), r in sorted(self.rows.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2], kv[0][3], kv[0][4])):
            lines.append(f"{plan:<12} {name:<34} {tag[:44]:<44} {sk:>6} {r['n']:>5} {r['worst']:>9.3f} {r['agg']:>9.3f}  {fl}")
        return "\n".join(lines)
